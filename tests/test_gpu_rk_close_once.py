"""Option rk_close_once: above 65 536 rows at d = 128 the rk4 drivers form a step's closing combination
P = y + h/8 k0 + 3h/8 k1 + 3h/8 k2 once - in the launch that already holds the four arrays (the last stage's dense product:
aux output; the SpMM of the adjoint's last stage: third output) - and the closing launch reads {1.0, P} instead of the
four terms.  P is formed with the multiply-add chain every kernel forms a combination with, so every comparison here is
torch.equal: whole solves with the option on against off, the dense launch's aux output and the SpMM's third output
against gode_lincomb_f32 of the same terms and coefficients."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPMM, GEMM_FWD, BWD_WGRAD = 0, 1, 4
PC = 2 << 8


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@contextlib.contextmanager
def options(**kw):
    from graph_odenet_amd import _lib
    lib = _lib.load()
    old = {k: lib.gode_get_option(k.encode()) for k in kw}
    try:
        for k, v in kw.items():
            assert lib.gode_set_option(k.encode(), v) == 0 and lib.gode_get_option(k.encode()) == v, k
        yield
    finally:
        for k, v in old.items():
            lib.gode_set_option(k.encode(), v)


@contextlib.contextmanager
def profiled(cap=512):
    """(kind, extra operand arrays) of the profiled launches issued in the body, in launch order."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    prof = lib.gode_prof_create(cap)
    assert prof
    out = []
    lib.gode_prof_enable(prof)
    try:
        yield out
        torch.cuda.synchronize()
        n = lib.gode_prof_count(prof)
        assert 0 < n < cap
        ms, extra, kinds = (ctypes.c_float * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int32 * n)()
        assert lib.gode_prof_read(prof, ms, None, None, extra, n) == n
        assert lib.gode_prof_kinds(prof, kinds, n) == n
        out.extend((int(k), int(e)) for k, e in zip(kinds, extra))
    finally:
        lib.gode_prof_enable(None)
        lib.gode_prof_destroy(prof)


def extras_of(launches, kind):
    return [e for k, e in launches if k == kind]


# ---------------------------------------------------------------------------------------------------------------------
# 1. whole solves, option on against off
# ---------------------------------------------------------------------------------------------------------------------
class _Problem:
    def __init__(self):
        from graph_odenet_amd import models, odeint as OI, synth
        g = synth.rmat_graph(17, 1 << 20, seed=1, device=dev())
        assert g.n_rows == 1 << 17
        torch.manual_seed(7)
        f = models.ODEfunc(128)
        with torch.no_grad():
            f.norm1.weight.uniform_(0.5, 1.5)
            f.norm1.bias.uniform_(-0.5, 0.5)
        f = f.to(dev())
        f.set_adj(g)
        self.f = f
        self.y0 = torch.randn(g.n_rows, 128, device=dev())
        self.a1 = torch.randn(g.n_rows, 128, device=dev())
        self.fwd, self.mk_adj, _ = OI._fields(f, self.y0)
        assert getattr(self.fwd, "rk4_native", None) is not None

    def solve(self):
        """gode_gcn_ode_rk4_forward on [0, 1] and gode_gcn_ode_rk4_adjoint back, 2 steps each: y(1); y(0), a(0), theta."""
        with torch.no_grad():
            y = [self.y0.clone()]
            self.fwd.rk4_native(y, 0.0, 1.0, 2)
            adj = self.mk_adj()
            comps = adj.new_state(y[0])
            comps[1].copy_(self.a1)
            adj.rk4_native(comps, 1.0, 0.0, 2)
            torch.cuda.synchronize()
            return y[0].clone(), comps[0].clone(), comps[1].clone(), adj.theta.clone()


@pytest.fixture(scope="module")
def problem():
    return _Problem()


@pytest.mark.parametrize("overlap", [1, 0])
def test_rk4_solves_bit_identical_with_the_closing_combination_formed_once(problem, overlap):
    """R-MAT 2^17 rows, d = 128, rk4 with 2 steps: y(1) of the forward solve and y, a, theta of the adjoint solve with
    rk_close_once 1 against 0, torch.equal, under both schedules.  The extra-array counts of the profiled launches show
    that the option changed what ran: the closing SpMM launches carry one pre-term (forward: 1 extra array instead of
    4; adjoint: 1 + 4 cotangent terms + Y2 + the third output = 7 instead of 4 + 4 + 1 = 9), the stage-3 one-pass dense
    launch one pre-term instead of four, and the last stage's forward product one more output."""
    p = problem
    res, seen = {}, {}
    for on in (1, 0):
        with options(rk_close_once=on, overlap=overlap):
            with profiled() as launches:
                res[on] = p.solve()
        seen[on] = launches
    for name, u, v in zip(("y(1)", "y(0)", "a(0)", "theta"), res[1], res[0]):
        assert torch.isfinite(u).all(), name
        assert torch.equal(u, v), "%s differs with rk_close_once (overlap %d)" % (name, overlap)
    assert not torch.equal(res[1][2], p.a1) and res[1][3].abs().max().item() > 0
    # forward solve: 8 Gf + 8 Sp; adjoint solve: 8 Gf, 8 Sp, 8 SpT, 8 one-pass dense launches
    nf = 16
    for on, sp3_f, sp3_a, gf3_f, gf3_a, bw3 in ((1, 1, 7, 4, 5, 1), (0, 4, 9, 3, 4, 4)):
        fwd_l, adj_l = seen[on][:nf], seen[on][nf:]
        assert {k for k, _ in seen[on]} == {SPMM, GEMM_FWD | PC, BWD_WGRAD | PC}, sorted({k for k, _ in seen[on]})
        assert extras_of(fwd_l, SPMM) == [0, 0, 0, sp3_f] * 2, (on, extras_of(fwd_l, SPMM))
        assert extras_of(fwd_l, GEMM_FWD | PC) == [0, 1, 2, gf3_f] * 2, (on, extras_of(fwd_l, GEMM_FWD | PC))
        # Sp(s) with s + 1 cotangent terms and Y2, then SpT(s)
        assert extras_of(adj_l, SPMM) == [2, 0, 3, 0, 4, 0, sp3_a, 0] * 2, (on, extras_of(adj_l, SPMM))
        # stages 2 and 3 also write their combined input (x_out), which the dense launch of the stage then reads
        assert extras_of(adj_l, GEMM_FWD | PC) == [0, 1, 3, gf3_a] * 2, (on, extras_of(adj_l, GEMM_FWD | PC))
        assert extras_of(adj_l, BWD_WGRAD | PC) == [0, 1, 0, bw3] * 2, (on, extras_of(adj_l, BWD_WGRAD | PC))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the dense launch alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_inputs():
    n, d = 65_569, 128                       # 2 049 tiles of 32 rows + 1 row; 4 098 of 16 rows + 1
    gen = torch.Generator().manual_seed(3)
    terms = [torch.randn(n, d, generator=gen).to(dev()) for _ in range(4)]
    W = (torch.randn(d + 1, d, generator=gen) / 11.0).to(dev())
    gamma = (torch.rand(d, generator=gen) + 0.5).to(dev())
    beta = (torch.rand(d, generator=gen) - 0.5).to(dev())
    h = 0.5
    xc = [1.0, np.float32(h * 1.0), np.float32(-h * 1.0), np.float32(h * 1.0)]              # the last stage's input
    ac = [1.0, np.float32(h / 8.0), np.float32(3.0 * h / 8.0), np.float32(3.0 * h / 8.0)]    # the closing combination
    return n, d, terms, W, gamma, beta, xc, ac


@pytest.mark.parametrize("fwd_pc", [3, 0], ids=["pc", "fp32"])
@pytest.mark.parametrize("with_xout", [True, False], ids=["xout", "noxout"])
def test_dense_launch_leaves_second_combination(dense_inputs, fwd_pc, with_xout):
    """n = 65 569 (ragged against the 32- and 16-row tiles), d = 128, 32 groups, 4 terms: aux_out of
    gode_gn_time_gemm_xout_aux_f32 is bit for bit gode_lincomb_f32 of the same terms under the second coefficients; S and
    x_out are bit for bit those of the entry point without aux_out; rows past n are not written.  Both kernels the large
    route can select: producer / consumer (fwd_pc 3) and fp32-MFMA (fwd_pc 0)."""
    from graph_odenet_amd import ops
    n, d, terms, W, gamma, beta, xc, ac = dense_inputs
    xt = list(zip([float(c) for c in xc], terms))
    want_aux = ops.lincomb_(torch.empty(n, d, device=dev()), list(zip([float(c) for c in ac], terms)))
    with options(fwd_pc=fwd_pc):
        with profiled() as plain:
            S0 = torch.empty(n, d, device=dev())
            X0 = torch.empty(n, d, device=dev()) if with_xout else None
            ops.gn_time_gemm(xt, n, d, 32, 1e-5, gamma, beta, W, True, 0.375, out=S0, x_out=X0)
        with profiled() as withaux:
            S1 = torch.empty(n, d, device=dev())
            X1 = torch.empty(n, d, device=dev()) if with_xout else None
            guard = torch.full((n + 3, d), float("nan"), device=dev())
            ops.gn_time_gemm(xt, n, d, 32, 1e-5, gamma, beta, W, True, 0.375, out=S1, x_out=X1,
                             aux_coefs=[float(c) for c in ac], aux_out=guard[:n])
    kind = GEMM_FWD | PC if fwd_pc else GEMM_FWD
    assert plain == [(kind, 3 + int(with_xout))] and withaux == [(kind, 4 + int(with_xout))], (plain, withaux)
    assert torch.equal(guard[:n], want_aux)
    assert bool(torch.isnan(guard[n:]).all()), "rows past n_rows were written"
    assert torch.isfinite(S0).all() and torch.equal(S1, S0)
    if with_xout:
        assert torch.equal(X1, X0)
        assert torch.equal(X0, ops.lincomb_(torch.empty(n, d, device=dev()), xt))


def test_dense_launch_refuses_what_it_cannot_form(dense_inputs):
    """Nothing is launched and GODE_E_UNSUPPORTED comes back where the selected kernel keeps no raw terms (three terms on
    the producer / consumer kernels; d = 64); an aux_out that is one of the terms is an argument error."""
    from graph_odenet_amd import _lib
    from graph_odenet_amd._lib import lincomb, ptr, stream_ptr
    lib = _lib.load()
    n, d, terms, W, gamma, beta, xc, ac = dense_inputs
    S = torch.zeros(n, d, device=dev())
    aux = torch.zeros(n, d, device=dev())

    def call(tl, dd, groups, aux_t):
        lc = lincomb(tl)
        coefs = (ctypes.c_float * 8)(*([1.0] * 8))
        return lib.gode_gn_time_gemm_xout_aux_f32(ctypes.byref(lc), n, dd, groups, 1e-5, ptr(gamma), ptr(beta), ptr(W), dd, 1,
                                                  0.5, ptr(S), None, coefs, ptr(aux_t), stream_ptr())
    three = [(1.0, terms[0]), (0.5, terms[1]), (0.25, terms[2])]
    assert call(three, d, 32, aux) == -5
    assert call(three, 64, 32, aux) == -5
    assert call(three, d, 32, terms[1]) == -4
    torch.cuda.synchronize()
    assert not S.any() and not aux.any(), "a refused call launched something"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the SpMM alone
# ---------------------------------------------------------------------------------------------------------------------
def test_spmm_third_output_and_pre_term_in_place():
    """70 001 rows, d = 128, one row of 1 000 non-zeros cut into several records (finished by the second launch): the
    launch with its pre-term {1.0, P} aliased to Y and the third output on gives Y, Y2 and the per-block column sums bit
    for bit those of the un-aliased launch with the four pre-terms, and a third output bit for bit gode_lincomb_f32 of
    the cotangent terms under the second coefficients."""
    from graph_odenet_amd import graph as G, ops
    n, d = 70_001, 128
    rs = np.random.RandomState(5)
    deg = rs.randint(0, 9, n)
    deg[123] = 1000
    rows = np.repeat(np.arange(n), deg)
    cols = rs.randint(0, n, rows.size)
    vals = rs.rand(rows.size).astype(np.float32) + 0.1
    g = G.from_coo(torch.from_numpy(rows).to(dev()), torch.from_numpy(cols).to(dev()), torch.from_numpy(vals).to(dev()),
                   n, n, split=128)
    assert g.n_long >= 1 and g.n_items > 65536
    assert 123 in g.long_rows[:, 0].tolist()
    gen = torch.Generator().manual_seed(9)
    X, b = torch.randn(n, d, generator=gen).to(dev()), torch.randn(d, generator=gen).to(dev())
    yk = [torch.randn(n, d, generator=gen).to(dev()) for _ in range(4)]
    ak = [torch.randn(n, d, generator=gen).to(dev()) for _ in range(4)]
    h = -0.5
    f32 = lambda v: float(np.float32(v))
    close = [1.0, f32(h / 8.0), f32(3.0 * h / 8.0), f32(3.0 * h / 8.0)]
    stage = [-1.0, -f32(h), f32(h), -f32(h)]                      # minus the last stage's input of the adjoint state
    alpha = f32(h / 8.0)
    pre4 = list(zip(close, yk))
    cot = list(zip(stage, ak))
    rows_cs = ops.spmm_y2_colsum_rows(g, d)
    assert rows_cs > 0
    cs0 = torch.empty(rows_cs, d, device=dev())
    Y0, Y20 = ops.spmm(g, X, bias=b, relu=True, cot_terms=cot, pre_terms=pre4, alpha=alpha, out2_colsum=cs0)
    P = ops.lincomb_(torch.empty(n, d, device=dev()), pre4)
    want3 = ops.lincomb_(torch.empty(n, d, device=dev()), list(zip(close, ak)))
    cs1 = torch.full((rows_cs, d), float("nan"), device=dev())
    Y3 = torch.full((n, d), float("nan"), device=dev())
    with profiled() as launches:
        Y1, Y21 = ops.spmm(g, X, bias=b, relu=True, out=P, cot_terms=cot, pre_terms=[(1.0, P)], alpha=alpha,
                           out2_colsum=cs1, cot_out=Y3, cot_out_coefs=close)
    assert launches == [(SPMM, 1 + 4 + 1 + 1)], launches
    assert Y1.data_ptr() == P.data_ptr()
    assert torch.isfinite(Y0).all() and torch.equal(Y1, Y0)
    assert torch.equal(Y21, Y20) and bool((Y20 != 0).any())
    assert torch.equal(cs1, cs0)
    assert torch.equal(Y3, want3)
