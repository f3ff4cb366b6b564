"""Option local_tail: gode_gcn_ode_rk4_forward integrates the isolated rows at the end of the state (gode_gcn_odefunc_t:
n_tail) over the whole solve in one row-local launch (csrc/gemm_pc.hip: gcn_local_tail_rk4_kernel) and runs its dense
launches on the rows before them (csrc/ode_driver.hip).  The kernel makes every stage with the statements of the DIAG dense
launches on the same numbers, so every comparison with the option off is torch.equal.

The graph: a core of 65 605 rows (above 65 536, not a multiple of 32: the tail starts inside a 32-row tile) - four random
entries per ordinary row; every 16th row diagonal-only in A but gathered by others (not isolated); every 16th row isolated,
scattered - followed by a tail of isolated rows of length 1, 31, 32, 33 (fewer tiles than blocks) or 20 011 (626 tiles for
128 blocks).  Diagonals are drawn from [0.5, 1.5] without 1.0.  The func struct is built directly, n_tail as given: the 1/8
share is the Python gate's business (tests/test_local_tail.py).

Bar against float64: 1e-5 of the largest reference magnitude, the suite's bar for the ODE function (test_gpu_kernels.py)."""
import ctypes

import pytest
import torch

from test_gpu_rk_close_once import dev, options

pytestmark = pytest.mark.gpu

N_CORE, D = 65_605, 128
TAILS = (1, 31, 32, 33, 20_011)
STEP_CAP = 16                                   # csrc/dense_pc.h: GODE_LOCAL_TAIL_MAX_STEPS
GEMM_FWD_PC, LOCAL_TAIL_PC, SPMM = 1 | (2 << 8), 12 | (2 << 8), 0
TOL = 1e-5

_graphs, _refs, _params = {}, {}, {}


def build_graph(n_tail):
    from graph_odenet_amd import graph as G
    n = N_CORE + n_tail
    gen = torch.Generator().manual_seed(n)
    ar = torch.arange(N_CORE)
    a_only, lone = ar % 16 == 1, ar % 16 == 2
    ordinary = ar[~a_only & ~lone]
    targets = ar[~lone]                                               # somebody gathers the a_only rows
    r = ordinary.repeat_interleave(4)
    c = targets[torch.randint(0, targets.numel(), (r.numel(),), generator=gen)]
    r = torch.cat([r, ordinary[:4096], ar[a_only] + 2])               # (i + 2, i): every a_only row is gathered for certain
    c = torch.cat([c, ordinary[:4096].flip(0), ar[a_only]])
    keep = r != c
    loops = torch.arange(n)
    key = torch.unique(torch.cat([r[keep], loops]) * n + torch.cat([c[keep], loops]))
    r, c = key // n, key % n
    v = (torch.rand(key.numel(), generator=gen) * 2 - 1) * 0.2
    on = r == c
    dv = 0.5 + torch.rand(int(on.sum()), generator=gen)
    dv[dv == 1.0] = 1.25
    v[on] = dv
    g = G.from_coo(r.to(dev()), c.to(dev()), v.to(dev()), n, n, split=256, coalesce=False)
    iso = g.isolated_rows().diag.cpu() != 0
    fa = g.diag_rows().diag.cpu() != 0
    assert g.isolated_tail() == n_tail and bool(iso[:N_CORE][lone].all()) and int(iso.sum()) == n_tail + int(lone.sum())
    assert torch.equal(fa[:N_CORE] & ~iso[:N_CORE], a_only)           # diagonal-only, not isolated
    tail_d = g.diag_rows().diag[N_CORE:].cpu()
    assert float(tail_d.min()) >= 0.5 and float(tail_d.max()) <= 1.5 and not bool((tail_d == 1.0).any())
    assert N_CORE % 32 != 0
    a64 = torch.sparse_coo_tensor(torch.stack([r, c]).to(dev()), v.double().to(dev()), (n, n)).coalesce()
    return g, a64


def graph_of(n_tail):
    if n_tail not in _graphs:
        _graphs[n_tail] = build_graph(n_tail)
    return _graphs[n_tail]


def params():
    if not _params:
        gen = torch.Generator().manual_seed(11)
        _params.update(W=(torch.randn(D + 1, D, generator=gen) / D ** 0.5).to(dev()),
                       b=(torch.rand(D, generator=gen) * 0.4 - 0.2).to(dev()),
                       gamma=(torch.rand(D, generator=gen) + 0.5).to(dev()),
                       beta=(torch.rand(D, generator=gen) - 0.5).to(dev()))
    return _params


def y0_of(n):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(n + 1)).to(dev())


def reference(n_tail, groups, n_steps, t0, t1):
    """The solve in float64 (3/8 rule), once per case; shared by both settings of local_tail and of overlap."""
    key = (n_tail, groups, n_steps, t0, t1)
    if key not in _refs:
        a64 = graph_of(n_tail)[1]
        p = {k: v.double() for k, v in params().items()}

        def f(t, x):
            xn = torch.nn.functional.group_norm(x, groups, p["gamma"], p["beta"], 1e-5) if groups else x
            s = torch.cat([torch.full((x.shape[0], 1), t, dtype=torch.float64, device=x.device), xn], 1) @ p["W"]
            return torch.relu(torch.sparse.mm(a64, s) + p["b"])
        y = y0_of(a64.shape[0]).double()
        h = (t1 - t0) / n_steps
        for i in range(n_steps):
            t = t0 + i * h
            k0 = f(t, y)
            k1 = f(t + h / 3, y + h / 3 * k0)
            k2 = f(t + 2 * h / 3, y + h * (k1 - k0 / 3))
            k3 = f(t + h, y + h * (k0 - k1 + k2))
            y = y + h * (k0 + 3 * k1 + 3 * k2 + k3) / 8
        _refs[key] = y
    return _refs[key]


def solve(n_tail, groups, n_steps, t0, t1, func_tail=None, profile=False):
    """gode_gcn_ode_rk4_forward on the graph with that tail; ws.S and the tail rows of the four stage buffers are NaN before
    it.  func_tail: the n_tail the func struct carries (default: the graph's).  -> y(t1), [(kind, rows)] of the launches."""
    from graph_odenet_amd import _lib
    from graph_odenet_amd.gcn_ode import _graph_struct
    lib = _lib.load()
    g = graph_of(n_tail)[0]
    n, p = g.n_rows, params()
    a, core = g.diag_rows(), g.transpose().isolated_rows()
    fs = _lib.GcnOdeFunc()
    fs.A, fs.AT = _graph_struct(g, D), _graph_struct(g.transpose(), D)
    fs.n, fs.d, fs.groups, fs.eps = n, D, groups, 1e-5
    fs.W, fs.b, fs.gamma, fs.beta = (p[k].data_ptr() for k in ("W", "b", "gamma", "beta"))
    fs.at_core_items, fs.at_n_core, fs.at_diag = core.items.data_ptr(), core.n_items, core.diag.data_ptr()
    fs.a_core_items, fs.a_n_core, fs.a_diag = a.items.data_ptr(), a.n_items, a.diag.data_ptr()
    fs.n_tail = n_tail if func_tail is None else func_tail
    y = y0_of(n)
    S = torch.full((n, D), float("nan"), device=dev())
    ky = [torch.zeros(n, D, device=dev()) for _ in range(4)]
    for k in ky:
        k[N_CORE:] = float("nan")
    ws = _lib.Rk4Workspace()
    ws.S = S.data_ptr()
    for i in range(4):
        ws.ky[i] = ky[i].data_ptr()
    res = ctypes.c_void_p()
    launches = []
    cap = 8 * n_steps + 8
    prof = lib.gode_prof_create(cap) if profile else None
    if profile:
        lib.gode_prof_enable(prof)
    try:
        rc = lib.gode_gcn_ode_rk4_forward(ctypes.byref(fs), _lib.ptr(y), ctypes.byref(res), ctypes.byref(ws), float(t0),
                                          float(t1), n_steps, _lib.stream_ptr())
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
    out = [t for t in [y] + ky if t.data_ptr() == res.value]
    assert len(out) == 1
    return out[0], launches


def check_case(n_tail, groups, n_steps, overlap, t0=0.0, t1=1.0):
    with torch.no_grad():
        with options(local_tail=1, overlap=overlap):
            on, _ = solve(n_tail, groups, n_steps, t0, t1)
        with options(local_tail=0, overlap=overlap):
            off, _ = solve(n_tail, groups, n_steps, t0, t1)
        ref = reference(n_tail, groups, n_steps, t0, t1)
        assert torch.isfinite(on).all() and torch.isfinite(off).all()
        err = float((on.double() - ref).abs().max() / ref.abs().max())
        print("tail %d groups %d steps %d overlap %d: err %.3g of the largest magnitude" % (n_tail, groups, n_steps, overlap, err))
        assert torch.equal(on, off)
        assert not torch.equal(on[N_CORE:], y0_of(on.shape[0])[N_CORE:])
        assert err < TOL


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("n_steps", [1, 2, 3, STEP_CAP + 1])
@pytest.mark.parametrize("groups", [32, 0])
@pytest.mark.parametrize("n_tail", TAILS)
def test_tail_launch_gives_the_bits_of_the_dense_launches(n_tail, groups, n_steps, overlap):
    """Every tail length x GroupNorm or none x step count (one more than a launch covers included) x stream placement: the
    solve with local_tail 1 equals the solve with 0 on ALL rows, and is within the bar of the float64 solve."""
    check_case(n_tail, groups, n_steps, overlap)


@pytest.mark.parametrize("overlap", [1, 0])
def test_backwards_in_time(overlap):
    """t1 < t0: negative step size, the stage times run down."""
    check_case(33, 32, 3, overlap, t0=1.0, t1=0.25)


def test_launch_lists():
    """n_tail = 0 in the func struct: the parent's launch list - Gf on n rows, Sp, eight launches per step, no tail launch -
    whatever the option says.  With the tail: one tail launch on n_tail rows first, then the same list with every dense launch
    on the core rows; local_tail 0 or fwd_pc 1 (not every dense launch has its DIAG form) keep the parent's list."""
    n_tail, steps = 20_011, 2
    n = N_CORE + n_tail
    g = graph_of(n_tail)[0]
    sp_rows = {g.n_items, g.diag_rows().n_items}
    with torch.no_grad():
        lists = {}
        for name, opts, ft in (("none_on", dict(local_tail=1), 0), ("none_off", dict(local_tail=0), 0),
                               ("tail_on", dict(local_tail=1), None), ("tail_off", dict(local_tail=0), None),
                               ("tail_fwd_pc1", dict(local_tail=1, fwd_pc=1), None)):
            with options(**opts):
                lists[name] = solve(n_tail, 32, steps, 0.0, 1.0, func_tail=ft, profile=True)
    parent = lists["none_off"][1]
    assert len(parent) == 8 * steps
    assert [k for k, _ in parent] == [GEMM_FWD_PC, SPMM] * (4 * steps) and all(r == n for k, r in parent if k == GEMM_FWD_PC)
    assert all(r in sp_rows for k, r in parent if k == SPMM)
    assert lists["none_on"][1] == parent and lists["tail_off"][1] == parent
    assert [k for k, _ in lists["tail_fwd_pc1"][1]].count(LOCAL_TAIL_PC) == 0
    assert all(r == n for k, r in lists["tail_fwd_pc1"][1] if (k & 0xff) == 1)
    got = lists["tail_on"][1]
    assert got[0] == (LOCAL_TAIL_PC, n_tail)
    assert got[1:] == [(k, N_CORE if k == GEMM_FWD_PC else r) for k, r in parent]
    for name in ("none_on", "tail_on", "tail_off"):
        assert torch.equal(lists[name][0], lists["none_off"][0]), name
    assert torch.isfinite(lists["tail_fwd_pc1"][0]).all()
