"""Option adjoint_tail: on the one-pass branch of gode_gcn_ode_rk4_adjoint the isolated rows at the end of the state
(gode_gcn_odefunc_t: n_tail, a_head_items) are recomputed, stage by stage, in a dense launch of their own
(csrc/gemm_pc.hip: gcn_adjoint_tail_kernel, gode_gcn_adjoint_tail_stage_f32) and Sp(g) runs on A's record list without them.
The launch makes every number with the statements of the pair it replaces - Gf, then the one-entry record of Sp(g) with the
cotangent epilogue - so k / y_new, dS, x_out and the third output are torch.equal, and it leaves per 8 rows the column-sum
row a block of Sp(g) leaves for 8 one-entry records, so the bias slot of theta keeps its bits as well.  The driver starts the
launch on a block boundary of A's record list: the first e = (-head records) mod 8 tail rows stay with Gf and Sp(g), and a
tail of no more than e rows keeps the parent's launches.  The core here has one record per row, 65 605 of them, so e = 3
(asserted): the solve-level tail of 1 row is the case that must NOT engage the route, and the tail of e + 1 = 4 rows is the
one whose tail launch runs on a single row; every longer tail must engage it (asserted through the rows nobody writes).

The graphs are those of tests/test_gpu_local_tail.py: a core of 65 605 rows (not a multiple of 32; scattered isolated rows
and rows that are diagonal-only on one side inside) followed by a tail of isolated rows, diagonals in [0.5, 1.5] without 1.0.

Bars.  Column sums: |fp32 sum - float64 sum| <= (n_rows - 1) 2^-24 sum|g| per column, the worst case of ANY order of n_rows - 1
fp32 additions (each rounds by at most 2^-24 of a partial sum, and no partial sum exceeds sum|g|); the float64 sums on either
side add 2^-53 of that and are not counted.  The bias slot against the float64 adjoint: 1e-5 of the slot's largest
magnitude, the bar of tests/test_gpu_local_tail.py against float64.  That comparison runs on parameters of its own
(margin_params): the adjoint holds the derivative of a relu, so where some z lies within rounding of 0 the float64 adjoint
takes one branch and an fp32 solve may take the other, and ONE such entry moves a bias-slot component by a whole cotangent
value (with the parameters of test_gpu_local_tail.py: 1.3e-3 of the slot's largest magnitude, the option on or off alike).
With |b| about 1 against |A S| of about 0.15 no z comes near 0 and the float64 adjoint is a reference.  The torch.equal
comparisons run on both parameter sets; on the ordinary one the masks are mixed in every column."""
import ctypes

import pytest
import torch

from test_gpu_local_tail import D, N_CORE, graph_of, params
from test_gpu_rk_close_once import dev, options

pytestmark = pytest.mark.gpu

LAUNCH_TAILS = (1, 31, 32, 33, 4_099)
E_HEAD = (-N_CORE) % 8                           # tail rows that fill the last block of 8 records of the head's list
SOLVE_TAILS = (1, E_HEAD + 1, 33, 20_011)       # not engaged; a launch of one row; two tiles; 626 tiles
GEMM_FWD_PC, ADJ_TAIL_PC, BWD_WGRAD_PC, SPMM = 1 | (2 << 8), 13 | (2 << 8), 4 | (2 << 8), 0
ZERO_COLS = (5, 64, 127)                         # W[:, c] = 0 and b[c] = 0: z is exactly 0 there
H = -1.0 / 3
STAGE_COEF = ([1.0], [1.0, H / 3], [1.0, -H / 3, H], [1.0, H, -H, H])       # the 3/8 rule's stage inputs
CLOSE_COEF = [1.0, H / 8, 3 * H / 8, 3 * H / 8]
TOL = 1e-5

_launch_params, _margin_params = {}, {}


def launch_params():
    """The parameters of test_gpu_local_tail.py with three output columns zeroed (weight column and bias)."""
    if not _launch_params:
        p = {k: v.clone() for k, v in params().items()}
        for c in ZERO_COLS:
            p["W"][:, c] = 0.0
            p["b"][c] = 0.0
        _launch_params.update(p)
    return _launch_params


def margin_params():
    """Every z = (A S)[i, c] + b[c] a whole unit away from 0: b[c] = +-(1 .. 1.1), alternating, S about 0.15."""
    if not _margin_params:
        gen = torch.Generator().manual_seed(12)
        sign = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0)
        _margin_params.update(W=(torch.randn(D + 1, D, generator=gen) * (0.1 / D ** 0.5)).to(dev()),
                              b=(sign * (1.0 + 0.1 * torch.rand(D, generator=gen))).to(dev()),
                              gamma=params()["gamma"], beta=params()["beta"])
    return _margin_params


def _spmm(g, items, n_items, X, Y, ep):
    from graph_odenet_amd import _lib
    return _lib.load().gode_spmm_csr_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(items), n_items,
                                         _lib.ptr(g.long_rows), g.n_long, _lib.ptr(g.partial(D)), _lib.ptr(X), D, _lib.ptr(Y), D,
                                         g.n_rows, D, ctypes.byref(ep), _lib.stream_ptr())


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("groups", [32, 0])
@pytest.mark.parametrize("n_tail", LAUNCH_TAILS)
def test_launch_gives_the_bits_of_the_pair(n_tail, groups, stage):
    """The tail launch against Gf on all rows followed by Sp(g) on A's whole list with Y2_scale, on the tail rows: k (stage 3:
    y_new), dS, x_out (stages 2 and 3) and the third output (stage 3) torch.equal; the rows before the tail of every output
    of the tail launch are NaN before and after it; z is exactly 0 in three columns and takes both signs elsewhere; the
    per-block column sums against float64 within the worst-case bound."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    g = graph_of(n_tail)[0]
    n, p = g.n_rows, launch_params()
    iso = g.transpose().isolated_rows().diag
    a_diag = g.diag_rows().diag
    nt = stage + 1
    gen = torch.Generator(device=dev()).manual_seed(100 * n_tail + 10 * stage + groups)
    yt = [torch.randn(n, D, generator=gen, device=dev()) for _ in range(nt)]
    ct = [torch.randn(n, D, generator=gen, device=dev()) for _ in range(nt)]
    yin = _lib.lincomb(list(zip(STAGE_COEF[stage], yt)))
    cot = _lib.lincomb([(-c, t) for c, t in zip(STAGE_COEF[stage], ct)])
    gam, bet = (_lib.ptr(p["gamma"]), _lib.ptr(p["beta"])) if groups else (None, None)
    t, alpha = 0.3, H / 8
    want_x = stage >= 2
    with torch.no_grad():
        # ---- the pair: Gf (stage 3: with the closing combination P into k), Sp(g) with the cotangent epilogue
        S, k0, dZ, dS0, x0, c30 = (torch.zeros(n, D, device=dev()) for _ in range(6))
        if stage < 3:
            rc = lib.gode_gn_time_gemm_xout_f32(ctypes.byref(yin), n, D, groups, 1e-5, gam, bet, _lib.ptr(p["W"]), D, 1, t,
                                                _lib.ptr(S), _lib.ptr(x0) if want_x else None, _lib.stream_ptr())
        else:
            rc = lib.gode_gn_time_gemm_xout_aux_f32(ctypes.byref(yin), n, D, groups, 1e-5, gam, bet, _lib.ptr(p["W"]), D, 1, t,
                                                    _lib.ptr(S), _lib.ptr(x0), (ctypes.c_float * 8)(*CLOSE_COEF), _lib.ptr(k0),
                                                    _lib.stream_ptr())
        assert rc == 0
        ep = _lib.SpmmEpilogue()
        ep.bias, ep.relu, ep.alpha = p["b"].data_ptr(), 1, 1.0
        ep.cot, ep.Y2 = cot, dZ.data_ptr()
        if stage == 3:
            ep.pre, ep.alpha, ep.cot_out = _lib.lincomb([(1.0, k0)]), alpha, c30.data_ptr()
            for j in range(4):
                ep.cot_out_coef[j] = CLOSE_COEF[j]
        assert _spmm(g, g.items, g.n_items, S, k0, ep) == 0           # no scale: dZ holds the unscaled g of every row
        g_unscaled = dZ[N_CORE:].clone()
        z_sign = S[N_CORE:] * a_diag[N_CORE:, None] + p["b"]
        if stage == 3:                                                # P again: Sp overwrote it in place
            assert lib.gode_gn_time_gemm_xout_aux_f32(ctypes.byref(yin), n, D, groups, 1e-5, gam, bet, _lib.ptr(p["W"]), D, 1, t,
                                                      _lib.ptr(S), _lib.ptr(x0), (ctypes.c_float * 8)(*CLOSE_COEF), _lib.ptr(k0),
                                                      _lib.stream_ptr()) == 0
        ep.Y2_scale, ep.Y2_scaled = iso.data_ptr(), dS0.data_ptr()
        assert _spmm(g, g.items, g.n_items, S, k0, ep) == 0
        # ---- the tail launch, every pointer at the first tail row
        off = N_CORE * D
        k1, dS1, x1, c31 = (torch.full((n, D), float("nan"), device=dev()) for _ in range(4))
        rows = int(lib.gode_gcn_adjoint_tail_colsum_rows(n_tail))
        assert rows == (n_tail + 7) // 8
        colsum = torch.full((rows + 1, D), float("nan"), device=dev())
        ty = _lib.lincomb([(c, v[N_CORE:]) for c, v in zip(STAGE_COEF[stage], yt)])
        tc = _lib.lincomb([(-c, v[N_CORE:]) for c, v in zip(STAGE_COEF[stage], ct)])
        last = stage == 3
        rc = lib.gode_gcn_adjoint_tail_stage_f32(
            ctypes.byref(ty), ctypes.byref(tc), n_tail, D, groups, 1e-5, gam, bet, _lib.ptr(p["W"]), t,
            _lib.ptr(a_diag[N_CORE:]), _lib.ptr(iso[N_CORE:]), _lib.ptr(p["b"]), _lib.ptr(k1[N_CORE:]), _lib.ptr(dS1[N_CORE:]),
            _lib.ptr(x1[N_CORE:]) if want_x else None, (ctypes.c_float * 4)(*CLOSE_COEF) if last else None, alpha if last else 0.0,
            (ctypes.c_float * 4)(*CLOSE_COEF) if last else None, _lib.ptr(c31[N_CORE:]) if last else None, _lib.ptr(colsum),
            _lib.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert off == N_CORE * D
        # z: exact zeros in the zeroed columns, both signs elsewhere
        assert bool((z_sign[:, list(ZERO_COLS)] == 0).all())
        if n_tail > 1:
            assert bool((z_sign > 0).any()) and bool((z_sign < 0).any())
        assert bool((g_unscaled[:, list(ZERO_COLS)] == 0).all()) and g_unscaled.abs().max().item() > 0
        for name, got, want, used in (("k", k1, k0, True), ("dS", dS1, dS0, True), ("x_out", x1, x0, want_x), ("cot_out", c31, c30, last)):
            assert torch.isnan(got[:N_CORE]).all(), name + ": a row before the tail was written"
            if used:
                assert torch.isfinite(want[N_CORE:]).all()
                assert torch.equal(got[N_CORE:], want[N_CORE:]), name
            else:
                assert torch.isnan(got).all(), name
        assert dS0[N_CORE:].abs().max().item() > 0 and not torch.equal(dS0[N_CORE:], g_unscaled)      # a_ii is never 1.0
        # column sums of the unscaled g: exactly `rows` rows written, each g[8q] + g[8q + 1] + .. in that order in fp32 (the
        # SpMM block's order), and their sum within the worst-case bound of float64
        assert torch.isfinite(colsum[:rows]).all() and torch.isnan(colsum[rows]).all()
        gp = torch.zeros(8 * rows, D, device=dev())
        gp[:n_tail] = g_unscaled
        seq = gp[0::8].clone()
        for j in range(1, 8):
            seq = seq + gp[j::8]
        assert torch.equal(colsum[:rows], seq)
        got = colsum[:rows].double().sum(0)
        want = g_unscaled.double().sum(0)
        bound = (n_tail - 1) * 2.0 ** -24 * g_unscaled.double().abs().sum(0)
        err = (got - want).abs()
        print("tail %d groups %d stage %d: colsum err / bound max %.3g" % (n_tail, groups, stage,
                                                                          float((err / bound.clamp_min(1e-300)).max()) if n_tail > 1 else 0.0))
        assert bool((err <= bound).all())


def test_launch_refuses_what_it_has_no_form_for():
    from graph_odenet_amd import _lib
    lib = _lib.load()
    p = launch_params()
    n = 64
    a = [torch.ones(n, D, device=dev()) for _ in range(10)]
    one = torch.ones(n, device=dev())
    cs = torch.zeros(2, D, device=dev())

    def call(nt, groups, last, d=D):
        ty, tc = _lib.lincomb([(1.0, a[j]) for j in range(nt)]), _lib.lincomb([(1.0, a[4 + j]) for j in range(nt)])
        cf = (ctypes.c_float * 4)(*CLOSE_COEF) if last else None
        return lib.gode_gcn_adjoint_tail_stage_f32(ctypes.byref(ty), ctypes.byref(tc), n, d, groups, 1e-5, None, None, _lib.ptr(p["W"]),
                                                   0.0, _lib.ptr(one), _lib.ptr(one), _lib.ptr(p["b"]), _lib.ptr(a[8]), _lib.ptr(a[9]),
                                                   None, cf, 0.1, cf, _lib.ptr(a[3]) if last else None, _lib.ptr(cs), _lib.stream_ptr())
    assert call(1, 32, False) == 0 and call(3, 0, False) == 0
    assert call(4, 32, False) != 0                    # four terms: the closed step only
    assert call(3, 32, True) != 0
    assert call(1, 16, False) != 0                    # 8 channels per group
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# whole adjoint solves
# ---------------------------------------------------------------------------------------------------------------------
_refs, _states = {}, {}


def state_of(n):
    if n not in _states:
        gen = torch.Generator().manual_seed(n + 3)
        _states[n] = (torch.randn(n, D, generator=gen).to(dev()), torch.randn(n, D, generator=gen).to(dev()))
    return _states[n]


def reference(n_tail, groups, n_steps):
    """The adjoint solve in float64 on margin_params() - d/dt [y, a, theta] = [f, -a^T df/dy, -a^T df/dtheta], 3/8 rule from t = 1 to t = 0 - once
    per case; shared by both settings of adjoint_tail and of overlap.  -> theta (the driver's layout)."""
    key = (n_tail, groups, n_steps)
    if key not in _refs:
        a64 = graph_of(n_tail)[1]
        n = a64.shape[0]
        names = ("W", "b", "gamma", "beta")
        p = [margin_params()[k].double().requires_grad_(True) for k in names]

        def aug(t, y, a):
            with torch.enable_grad():
                tt = torch.tensor(t, dtype=torch.float64, device=dev(), requires_grad=True)
                yy = y.detach().requires_grad_(True)
                xn = torch.nn.functional.group_norm(yy, groups, p[2], p[3], 1e-5) if groups else yy
                s = torch.cat([tt.expand(n, 1), xn], 1) @ p[0]
                f = torch.relu(torch.sparse.mm(a64, s) + p[1])
                grads = torch.autograd.grad(f, [yy, tt] + (p if groups else p[:2]), grad_outputs=-a, allow_unused=False)
            ga, gt, gp = grads[0], grads[1], list(grads[2:])
            if not groups:
                gp += [torch.zeros(D, dtype=torch.float64, device=dev())] * 2
            return f.detach(), ga, torch.cat([gp[0].flatten(), gp[1], gp[2], gp[3], gt.reshape(1)])
        y, a = (x.double() for x in state_of(n))
        th = torch.zeros((D + 1) * D + 3 * D + 1, dtype=torch.float64, device=dev())
        h = -1.0 / n_steps
        for i in range(n_steps):
            t = 1.0 + i * h
            k0 = aug(t, y, a)
            k1 = aug(t + h / 3, y + h / 3 * k0[0], a + h / 3 * k0[1])
            k2 = aug(t + 2 * h / 3, y + h * (k1[0] - k0[0] / 3), a + h * (k1[1] - k0[1] / 3))
            k3 = aug(t + h, y + h * (k0[0] - k1[0] + k2[0]), a + h * (k0[1] - k1[1] + k2[1]))
            y, a, th = (v + h * (q0 + 3 * q1 + 3 * q2 + q3) / 8 for v, q0, q1, q2, q3 in zip((y, a, th), k0, k1, k2, k3))
        _refs[key] = th
    return _refs[key]


def solve(n_tail, groups, n_steps, func_tail=None, profile=False, p=None):
    """gode_gcn_ode_rk4_adjoint from t = 1 to t = 0 on the graph with that tail, the func struct built directly.  Before it
    the tail rows of S, S2, dZ and of the stage buffers are NaN.  -> (y, a, theta), whether the tail rows of S, S2 and dZ
    (from the row the tail launch starts at) are still all NaN, [(kind, rows)] of the profiled launches, e."""
    from graph_odenet_amd import _lib, gcn_ode
    lib = _lib.load()
    g = graph_of(n_tail)[0]
    n, p = g.n_rows, p or params()
    a_core, core = g.diag_rows(), g.transpose().isolated_rows()
    fs = _lib.GcnOdeFunc()
    fs.A, fs.AT = gcn_ode._graph_struct(g, D), gcn_ode._graph_struct(g.transpose(), D)
    fs.n, fs.d, fs.groups, fs.eps = n, D, groups, 1e-5
    fs.W, fs.b, fs.gamma, fs.beta = (p[k].data_ptr() for k in ("W", "b", "gamma", "beta"))
    fs.at_core_items, fs.at_n_core, fs.at_diag = core.items.data_ptr(), core.n_items, core.diag.data_ptr()
    fs.a_core_items, fs.a_n_core, fs.a_diag = a_core.items.data_ptr(), a_core.n_items, a_core.diag.data_ptr()
    fs.n_tail = n_tail if func_tail is None else func_tail
    head = g.items[:g.n_items - n_tail]       # the head is a prefix of the list: the driver wants A.items itself
    assert torch.equal(head, g.items[g.items[:, 0].to(torch.int64) < N_CORE]) and head.data_ptr() == g.items.data_ptr()
    e = (-head.shape[0]) % 8                  # tail rows that fill the head's last block of 8 records: they stay with Sp(g)
    assert e == E_HEAD == 3
    if fs.n_tail:
        fs.a_head_items, fs.a_n_head = head.data_ptr(), head.shape[0]
    sh = gcn_ode._Shared(g, D, dev())
    ws = sh.workspace_struct(True, groups)
    assert ws.y2_colsum and ws.S2 and ws.X[0]
    ky, ka, _, _ = sh.stage_buffers(True)
    for buf in [sh.S, sh.S2, sh.dZ, sh.dS] + ky + ka + sh.X2:
        buf.zero_()
        buf[N_CORE:] = float("nan")
    y, a = (x.clone() for x in state_of(n))
    theta = torch.zeros(int(lib.gode_gcn_ode_theta_len(D)), device=dev())
    yr, ar = ctypes.c_void_p(), ctypes.c_void_p()
    cap = 64 * n_steps + 8
    prof = lib.gode_prof_create(cap) if profile else None
    launches = []
    if profile:
        lib.gode_prof_enable(prof)
    try:
        rc = lib.gode_gcn_ode_rk4_adjoint(ctypes.byref(fs), _lib.ptr(y), _lib.ptr(a), _lib.ptr(theta), ctypes.byref(yr),
                                          ctypes.byref(ar), ctypes.byref(ws), 1.0, 0.0, n_steps, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        if profile:
            cnt = lib.gode_prof_count(prof)
            assert 0 < cnt < cap
            ms, rows, kinds = (ctypes.c_float * cnt)(), (ctypes.c_int64 * cnt)(), (ctypes.c_int32 * cnt)()
            assert lib.gode_prof_read(prof, ms, None, rows, None, cnt) == cnt and lib.gode_prof_kinds(prof, kinds, cnt) == cnt
            launches = [(int(k), int(r)) for k, r in zip(kinds, rows)]
    finally:
        if profile:
            lib.gode_prof_enable(None)
            lib.gode_prof_destroy(prof)
    yo = [t for t in [y] + ky if t.data_ptr() == yr.value]
    ao = [t for t in [a] + ka if t.data_ptr() == ar.value]
    assert len(yo) == 1 and len(ao) == 1
    untouched = e < n_tail and all(bool(torch.isnan(b[N_CORE + e:]).all()) for b in (sh.S, sh.S2, sh.dZ))
    return (yo[0].clone(), ao[0].clone(), theta), untouched, launches, e


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("n_steps", [1, 2, 3])
@pytest.mark.parametrize("groups", [32, 0])
@pytest.mark.parametrize("n_tail", SOLVE_TAILS)
def test_solve_keeps_every_bit(n_tail, groups, n_steps, overlap):
    """adjoint_tail 1 against 0: y, a and every slot of theta torch.equal; the b slot of both within the bar of the float64
    adjoint; with the option on the tail rows of S, S2 and dZ are never written (NaN before and after) and nothing
    that is read holds a NaN (every result finite); two runs with the option on are bit-identical."""
    nW = (D + 1) * D
    with torch.no_grad():
        with options(adjoint_tail=1, overlap=overlap):
            on, on_untouched, _, e = solve(n_tail, groups, n_steps)
            again = solve(n_tail, groups, n_steps)[0]
            m_on = solve(n_tail, groups, n_steps, p=margin_params())[0][2]
        with options(adjoint_tail=0, overlap=overlap):
            off, off_untouched, _, _ = solve(n_tail, groups, n_steps)
            m_off = solve(n_tail, groups, n_steps, p=margin_params())[0][2]
    ref = reference(n_tail, groups, n_steps)
    for name, u, v, w in zip(("y", "a", "theta"), on, off, again):
        assert torch.isfinite(u).all() and torch.isfinite(v).all(), name
        assert torch.equal(u, w), "%s differs between two runs with the option on" % name
    scale = float(ref[nW:nW + D].abs().max())
    e_on = float((m_on[nW:nW + D].double() - ref[nW:nW + D]).abs().max()) / scale
    e_off = float((m_off[nW:nW + D].double() - ref[nW:nW + D]).abs().max()) / scale
    print("adjoint_tail tail %d groups %d steps %d overlap %d: bias slot error on %.3g off %.3g of its largest magnitude %.3g"
          % (n_tail, groups, n_steps, overlap, e_on, e_off, scale))
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert torch.equal(on[2][:nW], off[2][:nW]), "the weight slot"
    assert torch.equal(on[2][nW + D:], off[2][nW + D:]), "gamma, beta, a_t"
    assert torch.equal(on[2][nW:nW + D], off[2][nW:nW + D]), "the bias slot"
    assert on[2][:nW].abs().max().item() > 0 and on[2][-1].item() != 0 and on[2][nW:nW + D].abs().max().item() > 0
    assert on_untouched == (n_tail > E_HEAD) and not off_untouched    # engaged, except the 1-row tail: it fills the head's block
    assert torch.equal(m_on, m_off)
    assert scale > 0 and e_on < TOL and e_off < TOL


def test_launch_lists():
    """With the route: per stage one more dense launch, of the new kind, on n_tail rows; Gf on the rows before the tail; Sp(g)
    reporting A's whole record count.  n_tail = 0 in the func struct or the option off: the parent's list; fwd_pc 1: no tail launch."""
    n_tail, steps = 20_011, 2
    n = N_CORE + n_tail
    g = graph_of(n_tail)[0]
    with torch.no_grad():
        lists = {}
        for name, opts, ft in (("none_on", dict(adjoint_tail=1), 0), ("tail_off", dict(adjoint_tail=0), None),
                               ("tail_on", dict(adjoint_tail=1), None), ("tail_fwd_pc1", dict(adjoint_tail=1, fwd_pc=1), None),
                               ("tail_close0", dict(adjoint_tail=1, rk_close_once=0), None)):
            with options(overlap=0, **opts):
                lists[name] = solve(n_tail, 32, steps, func_tail=ft, profile=True)
    parent, e = lists["tail_off"][2], lists["tail_off"][3]
    n_head, n_launch = N_CORE + e, n_tail - e
    sp_rows = {g.n_items, g.transpose().n_items}
    assert [k for k, _ in parent] == [GEMM_FWD_PC] + [SPMM, SPMM, BWD_WGRAD_PC, GEMM_FWD_PC] * (4 * steps - 1) + [SPMM, SPMM, BWD_WGRAD_PC]
    assert all(r == n for k, r in parent if k != SPMM) and all(r in sp_rows for k, r in parent if k == SPMM)
    assert lists["none_on"][2] == parent
    pc1 = lists["tail_fwd_pc1"][2]                  # not every Gf on the producer / consumer kernel: no tail launch, every row
    assert len(pc1) == len(parent) and all((k & 0xff) != 13 for k, _ in pc1) and all(r == n for k, r in pc1 if (k & 0xff) == 1)
    got = lists["tail_on"][2]
    want = []
    for k, r in parent:
        if k == GEMM_FWD_PC:
            want += [(GEMM_FWD_PC, n_head), (ADJ_TAIL_PC, n_launch)]
        else:
            want.append((k, r))
    # each tail launch right behind its Gf and ahead of its Sp(g), which reports the whole record count
    assert got == want and len(got) == len(parent) + 4 * steps
    assert all(got[i + 1] == (SPMM, g.n_items) for i, x in enumerate(got) if x[0] == ADJ_TAIL_PC)
    # without the closing combination formed once the last stage keeps the full list; stages 0-2 go the new way
    c0 = lists["tail_close0"][2]
    assert [k for k, _ in c0].count(ADJ_TAIL_PC) == 3 * steps
    assert [r for k, r in c0 if k == GEMM_FWD_PC] == ([n_head] * 3 + [n]) * steps
    for u, v in zip(lists["none_on"][0], lists["tail_off"][0]):
        assert torch.equal(u, v)
    assert all(bool(torch.isfinite(u).all()) for u in lists["tail_fwd_pc1"][0])
