"""The fused GAT ODE function under message activations other than relu (outer_relu of gode_gat_act_t on
gode_gat_agg_f32_fwd / _bwd and gode_gat_agg_heads_f32_fwd;
`act, act_param` of gode_gat_odefunc_t; gat_ode.GatOdeField / GatOdeAdjointField) on the GPU.

Kernels: against a float64 restatement with torch's own activations and autograd on tests/gat_routes_design.py's designed
inputs, under that family's metric (errors relative to the ROW's own scale, all-zero rows exactly zero) and bound D.TOL = 2e-5
(tests/test_gpu_gat_act.py measures what float32 alone costs under it: at most 1.5e-6).  out = relu(m): relu is 1-Lipschitz, so
the bound that holds for the mean m, relative to the row's largest |m|, is the bound asked of relu(m).
The backward is held to the project's yardstick (noise_floor_check: slack 4, floor 1e-5 of the scale) under the same metric:
the error against float64 within 4 x the error of a float32 torch restatement of the same arithmetic + 1e-5.  D.TOL would
not do there: the mask leaves a row only the columns whose mean is positive, under tanh those with saturated messages, and
1 - y * y of a float32 y near 1 carries 6e-8 of absolute error whatever computes it - on S o = 16 the float32 restatement
itself is 2.6e-5 (one term) and 4.3e-5 (three terms) from float64 in dz, 5e-7 .. 1.5e-6 everywhere else.
The backward cases keep the designed means away from 0: a mask entry that float32 and float64 put on different sides of 0 is
no error of the kernel.  Their smallest non-zero |m| (float64, before any kernel runs) is 4.5e-5 .. 5.9e-4, asserted to be
at least KERNEL_MIN_ABS = 2e-5 - three times the 6e-6 that a float32 mean of row scale 4 can be off.

Fields and solves: against tests/gat_ode_act_ref.py (oracle.layers_ref with act=, relu outside) in float32 and float64, bar:
noise_floor_check of tests/test_gpu_gcn.py with its slack 4, on inputs designed as gat_ode_act_ref states and asserts.
Graphs and start states: tests/test_gpu_gat_backprop.py's T1 (37 nodes / 600 edges), T2 (golden gat_heads.npz), T3 (300 /
9 000: with H heads the raw-logit route)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixed_methods_ref as FR                                          # noqa: E402
import gat_ode_act_ref as G                                             # noqa: E402
import gat_routes_design as D                                           # noqa: E402
import test_gpu_gat_act as A                                            # noqa: E402  (activation codes, Check, route codes)
import test_gpu_gat_backprop as B                                       # noqa: E402  (graphs, x0_of, check, block_grads)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KERNEL_MIN_ABS = 2e-5
code = A.code


def routes():
    import test_gpu_gat_routes as R                                     # its cached designed EdgeGraphs and array helpers
    return R


# ---- the aggregation's restatement: float64, torch's activations, autograd -------------------------------------------------
def torch_act(act):
    c, p = act
    return {A.RELU: F.relu, A.IDENTITY: lambda z: z, A.LEAKY_RELU: lambda z: F.leaky_relu(z, p), A.ELU: lambda z: F.elu(z, p),
            A.TANH: torch.tanh, A.SIGMOID: torch.sigmoid}[c]


def agg_reference(d, v, act, cot=None, cot_scale=1.0, f64=torch.float64):
    """out = relu(m), m the layer's aggregate under `act`, in float64 over the compact nodes; with cot (a list of (coef,
    compact float32 tensor)) also the gradients of <out, cot_scale * sum coef cot> by autograd: dz per edge, da per edge with
    the maximum held fixed (no max path, as the kernels leave it), and their node sums.  Fields as gat_routes_design.reference
    fills them, plus m.  f64=torch.float32: the same arithmetic in single precision - what float32 alone costs."""
    s, t = torch.from_numpy(d.lut[d.src]), torch.from_numpy(d.lut[d.tgt])
    r, c = torch.from_numpy(d.lut[d.rows]), torch.from_numpy(d.cols)
    na, o = v.Ps.shape
    val = torch.ones(d.E, dtype=f64) if d.vals is None else torch.from_numpy(d.vals).to(f64)
    a32, amax = D.logits32(d, v)
    a = a32.to(f64).requires_grad_(True)
    z = ((v.Ps[s] + v.Pt[t]).to(f64) + v.bf.to(f64)).requires_grad_(True)      # gathered in fp32 (exact), then double
    w = torch.exp(a - amax.to(f64))
    y = torch_act(act)(z)
    we = val * w[c]
    den = torch.zeros(na, dtype=f64).index_add(0, r, we) + D.EPS
    m = torch.zeros(na, o, dtype=f64).index_add(0, r, we[:, None] * y[c]) / den[:, None]
    out = F.relu(m)
    ref = D.Design()
    ref.a32, ref.amax, ref.w, ref.den, ref.m, ref.out = a32, amax, w.detach(), den.detach(), m.detach(), out.detach()
    ref.edge_row = torch.empty(d.E, dtype=torch.int64)
    ref.edge_row[c] = r
    if cot is None:
        return ref
    g = cot_scale * sum(cf * ct.to(f64) for cf, ct in cot)
    (out * g).sum().backward()
    ref.dz, ref.da = z.grad, a.grad
    gm = torch.where(ref.m > 0, g, torch.zeros_like(g))                          # scales only: the terms without their cancellation
    dA, dsum = gm / ref.den[:, None], -(gm * ref.out).sum(1) / ref.den
    wed, yd = we.detach(), y.detach()
    ref.mag = torch.zeros(d.E, dtype=f64)
    ref.mag[c] = wed * ((dA[r] * yd[c]).abs().sum(1) + dsum[r].abs())
    ref.dPs = torch.zeros(na, o, dtype=f64).index_add_(0, s, ref.dz)
    ref.dPt = torch.zeros(na, o, dtype=f64).index_add_(0, t, ref.dz)
    ref.dA2 = torch.stack([torch.zeros(na, dtype=f64).index_add_(0, i, ref.da) for i in (s, t)], 1)
    ref.magA2 = torch.stack([torch.zeros(na, dtype=f64).index_add_(0, i, ref.mag) for i in (s, t)], 1)
    ref.magPs = torch.zeros(na, o, dtype=f64).index_add_(0, s, ref.dz.abs())
    ref.magPt = torch.zeros(na, o, dtype=f64).index_add_(0, t, ref.dz.abs())
    return ref


def forward_on_gpu(kind, o, act, split=None, offset=0, ode=True):
    """Logits and the ODE function's aggregation on a designed case -> arrays on the GPU and the route."""
    from graph_odenet_amd import ops
    R = routes()
    d, v = D.design(kind), D.values(kind, True, o)
    eg = R.edge_graph(kind, True, False, split)
    n, E = d.n, d.E
    g = D.Design()
    g.d, g.v, g.eg, g.n, g.E, g.o = d, v, eg, n, E, o
    g.Ps, g.Pt, g.A2 = R.full(v.Ps, eg, n), R.full(v.Pt, eg, n), R.full(v.A2, eg, n)
    g.bf, g.bw = v.bf.to(DEV), v.bw.to(DEV)
    g.proj = ops.gat_proj(g.Ps, g.Pt, g.A2)
    g.a, g.amax = R.sentinel(E), R.sentinel(1)
    ops.gat_logits(g.proj, g.bw, eg.src, eg.tgt, g.a, g.amax)
    g.out, g.w, g.den = R.sentinel(n, o, offset=offset), R.sentinel(E), R.sentinel(n)
    args = (eg, g.proj, o, g.bf, g.a, g.amax, D.EPS, g.out, g.w, g.den)
    g.route = ops.gat_agg_fwd_route(*args, act=act, ode=ode)
    assert g.route == ops.gat_agg_fwd_route(*args)                       # the dispatch does not depend on the activation
    ops.gat_agg_fwd(*args, act=act, ode=ode)
    return g


def check_forward(case, g, ref, ck=None):
    eg = g.eg
    own = ck is None
    ck = ck or A.Check(case)
    ck.true(torch.equal(g.a.cpu(), ref.a32) and g.amax.item() == ref.amax.item(), "logits bit for bit")
    out = g.out[eg.act].cpu()
    res = {"w": D.edge_error(g.w.cpu(), ref.w, ref.edge_row, ref.den.shape[0]), "den": D.node_error(g.den[eg.act].cpu(), ref.den),
           "out": D.node_error(out, ref.out, scale_src=ref.m)}
    for q, r in res.items():
        ck.add(g.route, q, *r)
    ck.true(bool((g.out[eg.inactive] == 0).all()) and bool((g.den[eg.inactive] == np.float32(D.EPS)).all()),
            "rows without edges: out 0, den eps")
    ck.true(bool((out >= 0).all()), "no negative output behind the outer relu")
    closed, opened = (ref.m < -1e-4), (ref.m > 1e-4)
    ck.true(bool(closed.any()) and bool((out[closed] == 0).all()), "some outputs are exactly 0: every clearly negative mean")
    ck.true(bool(opened.any()) and bool((out[opened] > 0).all()), "some outputs are positive: every clearly positive mean")
    if own:
        ck.done()


# ---- 1. the forward with the outer relu, route by route -----------------------------------------------------------------------
FWD_CASES = [("S", 16, None, code(1, 4)), ("S", 32, None, code(1, 8)), ("S", 64, None, code(1, 16)), ("S", 8, None, code(1, 2)),
             ("L", 24, None, code(3, 1)), ("L", 16, None, code(4, 4)), ("L", 16, D.SPLIT, code(4, 4))]


@pytest.mark.parametrize("name", ["elu", "tanh"])
@pytest.mark.parametrize("kind,o,split,route", FWD_CASES)
def test_forward_with_the_outer_relu_on_every_route(kind, o, split, route, name):
    """Prefetched at both widths of a row's lane group (o = 16, 32, 64: a wave per row; o = 8: four rows per wave), the lane
    group kernel, the record kernel without and with split rows (66 003 targets: the split rows are closed, and clamped, by
    the finishing launch)."""
    g = forward_on_gpu(kind, o, A.ACTS[name], split)
    assert g.route == route, (g.route, route)
    ref = agg_reference(g.d, g.v, A.ACTS[name])
    if split is not None:                                                # the rows the finishing launch writes have both signs
        rows = torch.from_numpy(g.d.lut[np.array([p for p, s in g.d.special.items() if s > D.SPLIT])])
        assert bool((ref.m[rows] < -1e-4).any()) and bool((ref.m[rows] > 1e-4).any())
    check_forward("%s %s o=%d%s" % (name, kind, o, " split" if split else ""), g, ref)


@pytest.mark.parametrize("name", list(A.ACTS))
def test_forward_every_activation_on_the_prefetched_route(name):
    g = forward_on_gpu("S", 16, A.ACTS[name])
    assert g.route == code(1, 4)
    ref = agg_reference(g.d, g.v, A.ACTS[name])
    ck = A.Check("%s S o=16" % name)
    if name == "sigmoid":                                                # positive messages: the outer relu is the identity
        assert bool((ref.m >= 0).all())
        for q, r in {"w": D.edge_error(g.w.cpu(), ref.w, ref.edge_row, ref.den.shape[0]),
                     "out": D.node_error(g.out[g.eg.act].cpu(), ref.out, scale_src=ref.m)}.items():
            ck.add(g.route, q, *r)
        ck.done()
        return
    check_forward("%s S o=16" % name, g, ref, ck)
    ck.done()


def wave_forward_case():
    return "S", 48, code(2, 1)


@pytest.mark.parametrize("name", ["elu", "tanh"])
def test_forward_wave_route(name):
    """Not among the issue's forward routes, but a forward form all the same: a width off the prefetched set."""
    kind, o, route = wave_forward_case()
    g = forward_on_gpu(kind, o, A.ACTS[name])
    assert g.route == route
    check_forward("%s %s o=%d" % (name, kind, o), g, agg_reference(g.d, g.v, A.ACTS[name]))


@functools.lru_cache(maxsize=None)
def heads_case(H=2, o=8, n=300, E=4500):
    """A random base graph whose H-fold graph has more than 8 192 edges (the raw-logit route's side of the threshold)."""
    from graph_odenet_amd import gat_heads
    from graph_odenet_amd.gat_layers import EdgeGraph
    gen = torch.Generator().manual_seed(77)
    src, tgt = torch.randint(0, n, (E,), generator=gen), torch.randint(0, n - 2, (E,), generator=gen)
    eg = EdgeGraph(src.to(DEV), tgt.to(DEV), G.mtgt(n, tgt).to(DEV))
    egv = gat_heads.heads_graph(eg, H)
    nv = n * H
    c = D.Design()
    c.H, c.o, c.nv, c.egv = H, o, nv, egv
    c.Ps, c.Pt = (torch.from_numpy(D.quarters(np.random.RandomState(5 + k), nv, o)) for k in range(2))
    c.A2 = torch.rand(nv, 2, generator=gen) * 2 - 1
    c.bw = torch.tensor([0.375, -0.25])
    assert egv.E == E * H > 8192
    return c


@pytest.mark.parametrize("name", ["elu", "tanh"])
def test_forward_heads_raw_logit_route(name):
    """gode_gat_agg_heads_f32_fwd with outer_relu: every virtual row shifted by its head's maximum, reduced in the kernel from the partial
    maxima of the raw-logit launch (HeadMax), relu outside."""
    from graph_odenet_amd import _lib, ops
    c = heads_case()
    egv, H, o, nv = c.egv, c.H, c.o, c.nv
    act = A.ACTS[name]
    f = dict(dtype=torch.float32, device=DEV)
    Ps, Pt, A2, bw = c.Ps.to(DEV), c.Pt.to(DEV), c.A2.to(DEV), c.bw.to(DEV)
    proj = ops.gat_proj(Ps, Pt, A2)
    a, w, den, out = (torch.full(s, 77.0, **f) for s in ((egv.E,), (egv.E,), (nv,), (nv, o)))
    scratch = torch.empty(max(_lib.load().gode_gat_heads_scratch_bytes(egv.E, H), 16), dtype=torch.uint8, device=DEV)
    ops.gat_logits_heads_raw(proj, egv.src, egv.tgt, H, a, scratch, bw=bw)
    ops.gat_agg_heads_fwd(egv, proj, o, torch.zeros(o, **f), a, scratch, H, D.EPS, out, w, den, act=act)
    # float64, per head
    sv, tv = egv.src.cpu().long(), egv.tgt.cpu().long()
    head = tv % H
    a32 = (c.A2[sv, 0] + c.A2[tv, 1]) + c.bw[head]
    assert torch.equal(a.cpu(), a32), "raw logits bit for bit"
    hmax = torch.stack([a32[head == h].max() for h in range(H)])
    wr = torch.exp(a32.double() - hmax[head].double())
    val = egv.Mt.val.cpu().double() if egv.Mt.val is not None else torch.ones(egv.E, dtype=torch.float64)
    we = val * wr
    dn = torch.zeros(nv, dtype=torch.float64).index_add_(0, tv, we) + D.EPS
    y = torch_act(act)((c.Ps[sv] + c.Pt[tv]).double())
    m = torch.zeros(nv, o, dtype=torch.float64).index_add_(0, tv, we[:, None] * y) / dn[:, None]
    ck = A.Check("%s heads raw" % name)
    rt = code(1, 2)
    ck.add(rt, "w", *D.edge_error(w.cpu(), wr, tv, nv))
    ck.add(rt, "den", *D.node_error(den.cpu(), dn))
    ck.add(rt, "out", *D.node_error(out.cpu(), F.relu(m), scale_src=m))
    oc = out.cpu()
    ck.true(bool((oc[m < -1e-4] == 0).all()) and bool((m < -1e-4).any()), "clearly negative means are exactly 0")
    ck.true(bool((oc[m > 1e-4] > 0).all()) and bool((m > 1e-4).any()), "clearly positive means are positive")
    ck.done()


# ---- 2. the backward with the masked cotangent under elu and tanh ------------------------------------------------------------
BWD_CASES = [("prefetched", "S", 16, None, False, code(1, 4)), ("wave", "S", 48, None, False, code(2, 1)),
             ("wave, an unaligned term", "S", 16, None, True, code(2, 1)), ("record", "L", 32, D.SPLIT, False, code(4, 8))]


@pytest.mark.parametrize("name", ["elu", "tanh"])
@pytest.mark.parametrize("label,kind,o,split,unaligned,route", BWD_CASES)
def test_backward_with_the_masked_cotangent(label, kind, o, split, unaligned, route, name):
    """cot of 1 and 3 terms at scale -1 and +1 against float64 autograd of relu(m): dz, da, the node sums - on the record
    route the target sums are the kernel's own (did_target_sums)."""
    from graph_odenet_amd import ops
    R = routes()
    act = A.ACTS[name]
    g = forward_on_gpu(kind, o, act, split)
    d, v, eg, n, E = g.d, g.v, g.eg, g.n, g.E
    fwd_ref = agg_reference(d, v, act)
    lo = fwd_ref.m[fwd_ref.m != 0].abs().min().item()
    print("%s %s o=%d %s: smallest non-zero |m| %.3e" % (label, kind, o, name, lo))
    assert lo >= KERNEL_MIN_ABS                                          # a condition on the inputs (module docstring)
    ck = A.Check("%s %s %s o=%d" % (name, label, kind, o))
    for terms in (1, 3):
        for scale in (-1.0, 1.0):
            cot_cpu = list(zip(v.coef[:terms], v.cot[:terms]))
            ref = agg_reference(d, v, act, cot_cpu, scale)
            cot = []
            for j, (cf, ct) in enumerate(cot_cpu):
                buf = R.full(ct, eg, n)
                if unaligned and j == terms - 1:                         # the last term one float off a 16-byte boundary
                    off = R.sentinel(n, o, offset=1)
                    off.copy_(buf)
                    buf = off
                    assert buf.data_ptr() % 16 == 4
                cot.append((cf, buf))
            dz, da, dPs, dPt, dA2 = R.sentinel(E, o), R.sentinel(E), R.sentinel(n, o), R.sentinel(n, o), R.sentinel(n, 2)
            kw = dict(dPt=dPt, dA2=dA2, cot_terms=cot, cot_scale=scale, act=act, ode=True)
            rt = ops.gat_agg_bwd_route(eg, g.proj, o, g.bf, g.w, g.den, g.out, dz, da, **kw)
            assert rt == route, (label, terms, rt, route)
            did = ops.gat_agg_bwd(eg, g.proj, o, g.bf, g.w, g.den, g.out, dz, da, **kw)
            assert did == ((route & 255) == 4)
            if did:                                                      # dPt and dA2[:, 1] are the record kernel's target sums
                ops.spmm(eg.Ms_inc, dz, out=dPs)
                ops.spmm(eg.Ms_inc, da.view(-1, 1), out=dA2[:, 0:1])
            else:
                ck.true(bool((dPt == A.SENT).all()) and bool((dA2 == A.SENT).all()), "dPt / dA2 untouched off the record route")
                ops.gat_scatter(eg.Ms_inc, eg.Mt_inc, dz, da, dPs, dPt, dA2)
            res = D.compare_backward(ref, dz.cpu(), da.cpu(), dPs[eg.act].cpu(), dPt[eg.act].cpu(), dA2[eg.act].cpu())
            r32 = agg_reference(d, v, act, cot_cpu, scale, f64=torch.float32)
            own = D.compare_backward(ref, r32.dz, r32.da, r32.dPs, r32.dPt, r32.dA2)
            for q, (err, exact) in res.items():
                bar = 4.0 * own[q][0] + 1e-5
                print("%s terms %d scale %+.0f %-4s err %.3e  float32 restatement %.3e  bar %.3e  zero rows exact %s"
                      % (ck.case, terms, scale, q, err, own[q][0], bar, exact))
                ck.true(err <= bar and exact, (terms, scale, q, err, bar, exact))
            ck.true(all(bool((x[eg.inactive] == 0).all()) for x in (dPs, dPt, dA2)), "node sums of rows without edges are 0")
            closed = (ref.m < 0)[ref.edge_row]                           # per edge and column: the target's mean is negative
            ck.true(bool(closed.any()) and bool((ref.dz[closed] == 0).all()) and bool((ref.dz[~closed] != 0).any()),
                    "the reference's mask closes some entries and opens others")
    ck.done()


# ---- 3. relu through the new entry points is the old entry points ---------------------------------------------------------------
@pytest.mark.parametrize("kind,o,split,route", [("S", 16, None, code(1, 4)), ("L", 16, D.SPLIT, code(4, 4)), ("S", 48, None, code(2, 1))])
def test_relu_through_the_ode_entry_points_is_the_old_entry_points(kind, o, split, route):
    from graph_odenet_amd import ops
    R = routes()
    old, new = forward_on_gpu(kind, o, None, split, ode=False), forward_on_gpu(kind, o, (A.RELU, 0.0), split, ode=True)
    assert old.route == new.route == route
    for q in ("out", "w", "den"):
        assert torch.equal(getattr(old, q), getattr(new, q)), q
    v, eg, n, E = old.v, old.eg, old.n, old.E
    cot = [(cf, R.full(ct, eg, n)) for cf, ct in zip(v.coef[:3], v.cot[:3])]
    res = []
    for kw in (dict(), dict(act=(A.RELU, 0.0), ode=True), dict(act=None, ode=True)):
        dz, da, dPt, dA2 = R.sentinel(E, o), R.sentinel(E), R.sentinel(n, o), R.sentinel(n, 2)
        args = (eg, old.proj, o, old.bf, old.w, old.den, old.out, dz, da)
        rt = ops.gat_agg_bwd_route(*args, dPt=dPt, dA2=dA2, cot_terms=cot, cot_scale=-1.0, **kw)
        did = ops.gat_agg_bwd(*args, dPt=dPt, dA2=dA2, cot_terms=cot, cot_scale=-1.0, **kw)
        res.append((rt, did, dz, da, dPt, dA2))
    for other in res[1:]:
        assert other[0] == res[0][0] == route and other[1] == res[0][1]
        for a, b in zip(other[2:], res[0][2:]):
            assert torch.equal(a, b)


# ---- the ODE function: product and restatement ---------------------------------------------------------------------------------
CONFIGS = {"T1": (16, 1), "T2": (64, 8), "T3": (16, 2)}


def product(gname, act_name, seed=5):
    d, H = CONFIGS[gname]
    n, src, tgt = B.graph(gname)
    f = G.make_func(d, H, act_name, seed).to(DEV)
    f.set_adj(src.to(DEV), tgt.to(DEV), G.mtgt(n, tgt).to(DEV))
    return f


def refs_of(f, gname, act_name):
    n, src, tgt = B.graph(gname)
    return [G.OdeRef(f, n, src, tgt, dt, G.ACTS[act_name]) for dt in (torch.float32, torch.float64)]


def names(f):
    return [k for k, _ in f.named_parameters()]


FIELD_MEMBERS = B.MEMBERS + ("fixed_forward_save", "fixed_backprop")


# ---- 4. field level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act_name", ["elu", "tanh"])
@pytest.mark.parametrize("gname", ["T1", "T2", "T3"])
def test_fields_one_evaluation_and_one_adjoint_stage(gname, act_name):
    d, H = CONFIGS[gname]
    f = product(gname, act_name)
    x0 = B.x0_of(gname, d)
    fields = f.gode_fields(x0.to(DEV))
    assert fields is not None, "gode_fields gave None: no fused field for this activation"
    fwd, mk_adj, plist = fields
    assert fwd.fused and fwd.small() and len(plist) == len(names(f))
    assert fwd.raw_logits() == (gname == "T3")
    for member in FIELD_MEMBERS:
        assert getattr(fwd, member) is not None, member
    n = x0.shape[0]
    gen = torch.Generator().manual_seed(3)
    k1, k2, a0, a1, a2 = (0.5 * torch.randn(n, d, generator=gen) for _ in range(5))
    t, c1, c2 = 0.375, 0.125, -0.25
    what = "%s d=%d H=%d %s " % (gname, d, H, act_name)
    # one evaluation
    fwd.prepare()
    k = torch.full((n, d), 77.0, device=DEV)
    fwd.eval(t, [[(1.0, x0.to(DEV))]], [k])
    want = []
    for ref in refs_of(f, gname, act_name):
        with torch.no_grad():
            want.append(ref(torch.tensor(t, dtype=ref.dtype), x0.to(ref.dtype)))
        if ref.dtype == torch.float64:
            G.assert_away_from_the_kink(ref, act_name, what + "eval")
    B.check(k, want[0], want[1], what + "k")
    assert bool((k == 0).any()) and bool((k > 0).any()) and bool((k >= 0).all())
    # one adjoint stage: a three-term state and a three-term adjoint
    adj = mk_adj()
    adj.prepare()
    dev = lambda x: x.to(DEV)                                            # noqa: E731
    terms = [[(1.0, dev(x0)), (c1, dev(k1)), (c2, dev(k2))], [(1.0, dev(a0)), (c1, dev(a1)), (c2, dev(a2))]]
    out = [torch.full((n, d), 77.0, device=DEV), torch.full((n, d), 77.0, device=DEV), torch.full((1,), 77.0, device=DEV),
           torch.full((adj.s.n_theta,), 77.0, device=DEV)]
    adj.eval(t, terms, out)
    got = dict(zip(names(f), adj.param_grads([None, None, None, out[3]])), k=out[0], k_a=out[1], k_at=out[2])
    want = []
    for ref in refs_of(f, gname, act_name):
        dt = ref.dtype
        x = (x0.to(dt) + c1 * k1.to(dt) + c2 * k2.to(dt)).requires_grad_(True)
        a = a0.to(dt) + c1 * a1.to(dt) + c2 * a2.to(dt)
        tt = torch.tensor(t, dtype=dt, requires_grad=True)
        fe = ref(tt, x)
        vj = torch.autograd.grad(fe, [tt, x] + list(ref.p), -a)
        want.append(dict(zip(ref.keys, vj[2:]), k=fe.detach(), k_a=vj[1], k_at=vj[0].reshape(1)))
        if dt == torch.float64:
            G.assert_away_from_the_kink(ref, act_name, what + "adjoint stage")
    for key in got:
        B.check(got[key], want[0][key], want[1][key], what + "stage " + key)


@pytest.mark.parametrize("method,kw", [("rk4", dict(step_size=0.25)), ("dopri5", dict(tol=1e-4))])
@pytest.mark.parametrize("gname,act_name", [("T1", "elu"), ("T2", "elu"), ("T3", "tanh")])
def test_c_drivers_issue_the_launches_of_the_per_stage_python_driver(gname, act_name, method, kw):
    """ODEBlock(adjoint=True): the C drivers against the per-stage Python drivers - the same kernels in the same order, so
    outputs, gradients and nfe agree bit for bit (as test_gpu_gat_backprop.test_adjoint_native_step_matches_python_driver)."""
    from graph_odenet_amd import odeint as OI, solver as PS
    from graph_odenet_amd.models import ODEBlock
    d, H = CONFIGS[gname]
    n, src, tgt = B.graph(gname)
    args = (src.to(DEV), tgt.to(DEV), G.mtgt(n, tgt).to(DEV))
    x0 = B.x0_of(gname, d).to(DEV)
    gout = torch.randn(n, d, generator=torch.Generator().manual_seed(4)).to(DEV)
    res = {}
    for native in (True, False):
        PS.DOPRI5_NATIVE = OI.NATIVE_RK4 = native
        try:
            blk = ODEBlock(G.make_func(d, H, act_name, seed=6), method=method, **kw).to(DEV)
            assert blk.odefunc.gc1.act is G.ACTS[act_name]
            out, gx, gp = B.block_grads(blk, x0, gout, args)
            res[native] = (out, gx, gp, blk.nfe)
        finally:
            PS.DOPRI5_NATIVE = OI.NATIVE_RK4 = True
    assert res[True][3] == res[False][3]
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for a, b in zip(res[True][2], res[False][2]):
        assert torch.equal(a, b)
    assert bool((res[True][0] != x0).any())


# ---- 5. solves -------------------------------------------------------------------------------------------------------------------
T3PTS = [0.0, 0.5, 1.0]
TOL = 1e-3


def product_solve(f, x0, Rw, method, adjoint, grad=True):
    from graph_odenet_amd import odeint as OI
    solve = OI.odeint_adjoint if adjoint else OI.odeint
    kw = dict(rtol=TOL, atol=TOL, method=method, options={"step_size": 0.25} if method != "dopri5" else None)
    if not grad:
        with torch.no_grad():
            return solve(f, x0.to(DEV), torch.tensor(T3PTS, device=DEV), **kw)
    f.zero_grad(set_to_none=True)
    x = x0.to(DEV).requires_grad_(True)
    out = solve(f, x, torch.tensor(T3PTS, device=DEV), **kw)
    assert out.grad_fn is not None
    (out * Rw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in f.parameters()]


def oracle_dopri5(ref, x0, Rw, trace, adjoint):
    """The oracle solver on the product's own attempt sequences, interval by interval as the product solves (each interval
    starts its own controller) -> [y, dL/dx0, dL/dparams...]."""
    from oracle import solver_ref as S
    dt = ref.dtype
    x = x0.detach().clone().to(dt).requires_grad_(True)
    S.REPLAY = [list(seq) for seq in trace]
    try:
        y, outs = x, [x]
        for i in range(1, len(T3PTS)):
            tt = torch.tensor([T3PTS[i - 1], T3PTS[i]], dtype=dt)
            solve = S.odeint_adjoint if adjoint else S.odeint
            y = solve(ref, y, tt, rtol=TOL, atol=TOL, method="dopri5")[1]
            outs.append(y)
        out = torch.stack(outs)
        (out * Rw.to(dt)).sum().backward()
        assert S.REPLAY == [], "the oracle did not consume the product's sequences"
    finally:
        S.REPLAY = None
    return [out.detach(), x.grad.clone()] + [p.grad.clone() for p in ref.p]


SOLVE_CASES = [(g, "elu") for g in ("T1", "T2", "T3")] + [("T1", a) for a in ("tanh", "identity", "sigmoid", "leaky_relu")]


@pytest.mark.parametrize("method", ["rk4", "euler", "dopri5"])
@pytest.mark.parametrize("gname,act_name", SOLVE_CASES)
def test_solves_against_autograd_through_the_oracle(gname, act_name, method, monkeypatch):
    """t = [0, .5, 1]: rk4 and euler at step 0.25, dopri5 at tol 1e-3 on the product's own accepted steps; odeint (the fused
    backprop sweep) and odeint_adjoint; y, dL/dx0 and every parameter gradient."""
    from graph_odenet_amd import solver
    d, H = CONFIGS[gname]
    f = product(gname, act_name)
    assert f.gode_fields(B.x0_of(gname, d).to(DEV)) is not None, "gode_fields gave None: no fused field for this activation"

    def boom(self, t, x):
        raise AssertionError("ODEfunc.forward was called: the solve left the fused fields")
    n, src, tgt = B.graph(gname)
    x0 = B.x0_of(gname, d)
    Rw = torch.randn((3,) + tuple(x0.shape), generator=torch.Generator().manual_seed(4))
    keys = ["y", "x"] + names(f)
    for adjoint in (False, True):
        what = "%s d=%d H=%d %s %s %s " % (gname, d, H, act_name, method, "adjoint" if adjoint else "backprop")
        solver.TRACE = []
        try:
            with monkeypatch.context() as mp:
                if not adjoint:                                          # the sweep never calls the module
                    mp.setattr(type(f), "forward", boom)
                got = product_solve(f, x0, Rw, method, adjoint)
            trace = solver.TRACE
        finally:
            solver.TRACE = None
        assert torch.equal(got[0], product_solve(f, x0, Rw, method, adjoint, grad=False)), "forward differs under no_grad"
        if adjoint:                                                      # the second call (captured and replayed where eligible)
            again = product_solve(f, x0, Rw, method, adjoint)
            for a, b in zip(got, again):
                assert torch.equal(a, b), what + "second call"
        made = []

        def mk(dt):
            made.append(G.OdeRef(f, n, src, tgt, dt, G.ACTS[act_name]))
            return made[-1]
        if method == "dopri5":
            assert len(trace) >= 2 and all(any(a[1] for a in seq) for seq in trace)
            want = [oracle_dopri5(mk(dt), x0, Rw, trace, adjoint) for dt in (torch.float32, torch.float64)]
        else:
            runs = FR.reference_runs(mk, x0, T3PTS, Rw, method, 0.25, adjoint)
            want = [[o, gx] + gp for o, gx, gp in runs]
        G.assert_away_from_the_kink(made[1], act_name, what)
        for key, g, w32, w64 in zip(keys, got, want[0], want[1]):
            B.check(g.reshape(w64.shape), w32, w64, what + key)


# ---- 6. the plan token ------------------------------------------------------------------------------------------------------------
def test_changing_the_activation_between_captured_solves(monkeypatch):
    """One module, captured rk4 solves under elu, then gc1.act = tanh: tanh's result, not a replay of elu's graph."""
    from graph_odenet_amd import odeint as OI
    x = B.x0_of("T1", 16).to(DEV)
    t = torch.tensor([0.0, 1.0], device=DEV)

    def solve(f):
        with torch.no_grad():
            return OI.odeint_adjoint(f, x, t, method="rk4", options={"step_size": 0.25})[1].clone()
    monkeypatch.setattr(OI, "GRAPH_CAPTURE_MAX_ELEMS", 0)
    eager = {name: solve(product("T1", name)) for name in ("elu", "tanh")}
    assert not torch.equal(eager["elu"], eager["tanh"])
    monkeypatch.setattr(OI, "GRAPH_CAPTURE_MAX_ELEMS", 1 << 21)
    f = product("T1", "elu")
    for _ in range(3):
        assert torch.equal(solve(f), eager["elu"])
    f.gc1.act = torch.tanh
    for _ in range(3):
        assert torch.equal(solve(f), eager["tanh"]), "a solve after gc1.act changed replayed the old activation"
    f.gc1.act = F.elu
    assert torch.equal(solve(f), eager["elu"])
    plans = OI.plans_of(f)
    assert len(plans) == 2 and all(p.gf is not None for p in plans.values())


# ---- 7. off the launch-bound route ------------------------------------------------------------------------------------------------
def test_large_graph_one_evaluation_and_one_adjoint_stage():
    """66 000 nodes, d = 16, one head, elu: the record kernels (one target with 5 000 edges: split rows) and the separate
    dense launches.  One call each, against float64."""
    from graph_odenet_amd import ops
    n, E, d = 66_000, 200_000, 16
    gen = torch.Generator().manual_seed(31)
    src, tgt = torch.randint(0, n, (E,), generator=gen), torch.randint(0, n, (E,), generator=gen)
    tgt[:5000] = 7
    f = G.make_func(d, 1, "elu").to(DEV)
    f.set_adj(src.to(DEV), tgt.to(DEV), G.mtgt(n, tgt).to(DEV))
    x0 = 0.5 * torch.randn(n, d, generator=gen)
    a0 = torch.randn(n, d, generator=gen)
    fields = f.gode_fields(x0.to(DEV))
    assert fields is not None, "gode_fields gave None: no fused field for this activation"
    fwd, mk_adj, _ = fields
    assert fwd.fused and not fwd.small()
    s, w = fwd.s, fwd.w
    k = torch.full((n, d), 77.0, device=DEV)
    rt = ops.gat_agg_fwd_route(s.eg, w.proj, d, s.bf, w.a, w.amax, s.eps, k, w.wgt, w.den, act=s.act, ode=True)
    assert rt == code(4, 4) and s.eg.Mt.n_long > 0, (rt, s.eg.Mt.n_long)
    t = 0.375
    adj = mk_adj()
    adj.prepare()
    out = [k, torch.full((n, d), 77.0, device=DEV), torch.full((1,), 77.0, device=DEV), torch.full((adj.s.n_theta,), 77.0, device=DEV)]
    adj.eval(t, [[(1.0, x0.to(DEV))], [(1.0, a0.to(DEV))]], out)
    k2 = torch.full((n, d), 77.0, device=DEV)
    fwd.eval(t, [[(1.0, x0.to(DEV))]], [k2])
    assert torch.equal(k2, out[0])
    got = dict(zip(names(f), adj.param_grads([None, None, None, out[3]])), k=out[0], k_a=out[1], k_at=out[2])
    want = []
    for dt in (torch.float32, torch.float64):
        ref = G.OdeRef(f, n, src, tgt, dt, F.elu)
        x = x0.to(dt).requires_grad_(True)
        tt = torch.tensor(t, dtype=dt, requires_grad=True)
        fe = ref(tt, x)
        vj = torch.autograd.grad(fe, [tt, x] + list(ref.p), -a0.to(dt))
        want.append(dict(zip(ref.keys, vj[2:]), k=fe.detach(), k_a=vj[1], k_at=vj[0].reshape(1)))
        if dt == torch.float64:
            G.assert_away_from_the_kink(ref, "elu", "66 000 nodes")
    for key in got:
        B.check(got[key], want[0][key], want[1][key], "66 000 nodes elu " + key)


# ---- 8. what stays outside ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["T1", "T3"])
def test_a_lambda_has_no_fused_field_and_elu_never_builds_the_autograd_field(gname, monkeypatch):
    from graph_odenet_amd import odeint as OI
    d, H = CONFIGS[gname]
    x0 = B.x0_of(gname, d).to(DEV)
    f = product(gname, "elu")
    G.set_act(f, lambda v: F.elu(v))
    assert f.gode_fields(x0) is None
    f = product(gname, "elu")

    class Never:
        def __init__(self, *a, **k):
            raise AssertionError("AutogradField was constructed for an activation the kernels restate")
    monkeypatch.setattr(OI, "AutogradField", Never)
    monkeypatch.setattr(OI, "AutogradAdjointField", Never)
    t = torch.tensor([0.0, 1.0], device=DEV)
    for solve, kw in ((OI.odeint, dict(method="rk4", options={"step_size": 0.5})), (OI.odeint_adjoint, dict(method="rk4", options={"step_size": 0.5})),
                      (OI.odeint, dict(rtol=1e-3, atol=1e-3)), (OI.odeint_adjoint, dict(rtol=1e-3, atol=1e-3))):
        x = x0.clone().requires_grad_(True)
        out = solve(f, x, t, **kw)
        out[1].sum().backward()
        assert bool(torch.isfinite(x.grad).all())
