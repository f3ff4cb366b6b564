"""Launch order of the C drivers in csrc/ode_driver.hip on the large route, through the public binding only.

A uniform random graph of 65 600 rows (just above the 65 536-row boundary below which the launch-bound kernels and the
merged stage-closing launch take over, and far too small to be renumbered), about 8 non-zeros per row, widths 128 (one-pass
VJP + weight gradient, closing combination formed once) and 64 (separate Gb and Wg), 2 rk4 steps.  Every case asserts the
COMPLETE ordered list of profiled launches - kind (GODE_PROF_* & 0xff) and the count of extra operand arrays - so a
driver that issued the same launches in another order, or fed one of them another term list, fails here even where the
numbers would still agree.  The orders follow from the schedule (ode_driver.hip's header); the extra counts at
d = 128 are those of tests/test_gpu_rk_close_once.py, the others were recorded from the drivers as they stood before
their launch sequences were folded into shared helpers.  Bits: forward-save ends where the plain forward solve does, and
the adjoint gives the same y, a, theta under both schedules (overlap 1 / 0)."""
import pytest
import torch

from test_gpu_rk_close_once import dev, options, profiled

pytestmark = pytest.mark.gpu

N_ROWS, N_STEPS = 65_600, 2
KIND = {"Sp": 0, "SpT": 0, "Gf": 1, "Gb": 2, "Wg": 3, "BW": 4}


def launches_of(names, extras):
    assert len(names) == len(extras), (len(names), len(extras))
    return [(KIND[k], e) for k, e in zip(names, extras)]


def seen(launches, what):
    got = [(k & 0xff, e) for k, e in launches]
    print(what, "kinds", [k for k, _ in got], "extras", [e for _, e in got])
    return got


def check(launches, names, extras, what):
    assert seen(launches, what) == launches_of(names, extras), what


@pytest.fixture(scope="module")
def graph():
    from graph_odenet_amd import graph as G
    gen = torch.Generator().manual_seed(65_600)
    rows = torch.arange(N_ROWS).repeat_interleave(7)
    cols = torch.randint(0, N_ROWS, (rows.numel(),), generator=gen)
    ar = torch.arange(N_ROWS)
    key = torch.unique(torch.cat([rows, ar]) * N_ROWS + torch.cat([cols, ar]))           # self-loops, duplicates removed
    r, c = key // N_ROWS, key % N_ROWS
    v = 1.0 / torch.bincount(r, minlength=N_ROWS).to(torch.float32)[r]                    # row-normalised
    return G.from_coo(r.to(dev()), c.to(dev()), v.to(dev()), N_ROWS, N_ROWS, coalesce=False)


class _Problem:
    """Fields as tests/test_gpu_rk_close_once.py::_Problem obtains them."""

    def __init__(self, g, d):
        from graph_odenet_amd import models, odeint as OI
        torch.manual_seed(7 + d)
        f = models.ODEfunc(d)
        with torch.no_grad():
            f.norm1.weight.uniform_(0.5, 1.5)
            f.norm1.bias.uniform_(-0.5, 0.5)
        f = f.to(dev())
        f.set_adj(g)
        self.f, self.d = f, d
        gen = torch.Generator().manual_seed(d)
        self.y0 = torch.randn(N_ROWS, d, generator=gen).to(dev())
        self.a1 = torch.randn(N_ROWS, d, generator=gen).to(dev())
        self.fwd, self.mk_adj, _ = OI._fields(f, self.y0)
        assert getattr(self.fwd, "rk4_native", None) is not None
        assert getattr(self.fwd, "row_order", None) is None, "the graph must run in its given node order"
        self._rec = None

    def records(self):
        """(records of gode_gcn_ode_rk4_forward_save over [0, 1], y(1), its launches): run once, shared, left unchanged."""
        if self._rec is None:
            with torch.no_grad():
                rec = torch.empty((N_STEPS, 5, N_ROWS, self.d), device=dev())
                rec[0, 0].copy_(self.y0)
                y_end = torch.empty_like(self.y0)
                with profiled() as launches:
                    self.fwd.rk4_forward_save(rec[0, 0], y_end, rec, 0.0, 1.0, N_STEPS, 0, N_STEPS)
            self._rec = (rec, y_end, launches)
        return self._rec


@pytest.fixture(scope="module")
def problems(graph):
    made = {}

    def get(d):
        if d not in made:
            made[d] = _Problem(graph, d)
        return made[d]
    yield get
    made.clear()


# extra operand arrays per launch of one step / one stage sequence (see the module docstring for where they come from)
FWD_EXTRAS = {128: [0, 0, 1, 0, 2, 0, 4, 1],          # Gf(3) also leaves the closing combination, Sp(3) reads it alone
              64: [0, 0, 1, 0, 2, 0, 3, 4]}
SAVE_EXTRAS = {128: [0, 0, 1, 0, 2, 0, 4, 1],
               64: [0, 0, 1, 0, 2, 0, 3, 4]}


@pytest.mark.parametrize("d", [128, 64])
def test_forward_and_forward_save(problems, d):
    """gode_gcn_ode_rk4_forward and gode_gcn_ode_rk4_forward_save: Gf, Sp four times per step, and the same y(1)."""
    p = problems(d)
    names = ["Gf", "Sp"] * 4 * N_STEPS
    with torch.no_grad():
        y = [p.y0.clone()]
        with profiled() as launches:
            p.fwd.rk4_native(y, 0.0, 1.0, N_STEPS)
    rec, y_end, save_launches = p.records()
    got, got_save = seen(launches, "forward d=%d" % d), seen(save_launches, "forward-save d=%d" % d)
    assert got == launches_of(names, FWD_EXTRAS[d] * N_STEPS)
    assert got_save == launches_of(names, SAVE_EXTRAS[d] * N_STEPS)
    assert torch.isfinite(y[0]).all() and not torch.equal(y[0], p.y0)
    assert torch.equal(y_end, y[0])
    assert torch.equal(rec[0, 0], p.y0)


# per step, after the leading Gf(0): stages 0..3 of  Sp, SpT, dense VJP ..., Gf of the NEXT stage
ADJ_NAMES = {128: ["Sp", "SpT", "BW", "Gf"], 64: ["Sp", "SpT", "Wg", "Gf", "Gb"]}
ADJ_EXTRAS = {128: [[2, 0, 0, 1], [3, 0, 1, 3], [4, 0, 0, 5], [7, 0, 1, 0]],
              64: [[2, 0, 0, 1, 0], [3, 0, 1, 3, 1], [4, 0, 0, 4, 0], [9, 0, 0, 0, 4]]}


@pytest.mark.parametrize("d", [128, 64])
def test_adjoint_both_schedules(problems, d):
    """gode_gcn_ode_rk4_adjoint from y(1) back: a leading Gf, then per stage Sp, SpT, the dense VJP launch(es) and the
    next stage's Gf (none after the last stage) - the same issue order with and without the side stream - and
    torch.equal results under both."""
    p = problems(d)
    y1 = p.records()[1]
    names, extras = ["Gf"], [0]
    for g in range(4 * N_STEPS):
        nm, ex = list(ADJ_NAMES[d]), list(ADJ_EXTRAS[d][g % 4])
        if g + 1 == 4 * N_STEPS:
            i = nm.index("Gf")
            del nm[i], ex[i]
        names += nm
        extras += ex
    res = {}
    for overlap in (1, 0):
        with options(overlap=overlap), torch.no_grad():
            adj = p.mk_adj()
            comps = adj.new_state(y1)
            comps[1].copy_(p.a1)
            with profiled() as launches:
                adj.rk4_native(comps, 1.0, 0.0, N_STEPS)
            res[overlap] = (comps[0].clone(), comps[1].clone(), adj.theta.clone())
        check(launches, names, extras, "adjoint d=%d overlap=%d" % (d, overlap))
    for name, u, v in zip(("y", "a", "theta"), res[1], res[0]):
        assert torch.isfinite(u).all(), name
        assert torch.equal(u, v), "%s differs between the schedules" % name
    assert not torch.equal(res[1][1], p.a1) and res[1][2].abs().max().item() > 0


# reverse sweep, stages 3..0 of a step
BP_NAMES = {128: ["SpT", "BW"], 64: ["SpT", "Gb", "Wg"]}
BP_EXTRAS = {128: [[0, 3], [0, 2], [0, 1], [0, 4]],                          # stage 1 adds abar + Ybar_2..4 into abar_n
             64: [[0, 3, 3], [0, 2, 2], [0, 1, 1], [0, 4, 0]]}


@pytest.mark.parametrize("d", [128, 64])
def test_backprop_sweep(problems, d):
    """gode_gcn_ode_rk4_backprop over the two records: per stage SpT, then the dense VJP launch(es)."""
    p = problems(d)
    rec = p.records()[0]
    names, extras = [], []
    for _ in range(N_STEPS):
        for s in (3, 2, 1, 0):
            names += BP_NAMES[d]
            extras += BP_EXTRAS[d][3 - s]
    with torch.no_grad():
        a = p.a1.clone()
        theta = torch.zeros((d + 1) * d + 3 * d + 1, device=dev())
        with profiled() as launches:
            res = p.fwd.rk4_backprop(rec, a, theta, 0.0, 1.0, N_STEPS, 0, N_STEPS)
    check(launches, names, extras, "backprop d=%d" % d)
    assert torch.isfinite(res).all() and torch.isfinite(theta).all() and theta.abs().max().item() > 0


# stages 1..6: from three terms on Gf writes the combined input out, which Gb and Wg then read as one array
DP_EXTRAS = [[1, 3, 0, 1, 1], [3, 4, 0, 0, 0], [4, 5, 0, 0, 0], [5, 6, 0, 0, 0], [6, 7, 0, 0, 0], [6, 7, 0, 0, 0]]


def test_dopri5_adjoint_step(problems):
    """One gode_gcn_ode_dopri5_step_adjoint at d = 64: stages 1..6, each Gf, Sp, SpT, Gb, Wg."""
    p = problems(64)
    with torch.no_grad():
        adj = p.mk_adj()
        y = adj.new_state(p.records()[1])
        y[1].copy_(p.a1)
        kk = adj.alloc_like(y, 7)
        y1 = adj.alloc_like(y, 1)[0]
        adj.eval(1.0, [[(1.0, c)] for c in y], kk[0])               # the FSAL stage the caller hands in
        with profiled() as launches:
            sums = adj.dopri5_step_native(y, kk, y1, 1.0, -0.05, 1e-3, 1e-3)
    check(launches, ["Gf", "Sp", "SpT", "Gb", "Wg"] * 6, sum(DP_EXTRAS, []), "dopri5 adjoint step d=64")
    assert torch.isfinite(sums).all() and torch.isfinite(y1[0]).all() and torch.isfinite(y1[1]).all()
