"""The message activation of the edge-attention kernels (csrc/edge.hip: the ActAny instantiations behind
the gode_gat_act_t argument of gode_gat_agg_f32_fwd / _bwd)
against a float64 restatement, route by route, and the layers that reach them.

Restatement.  `reference` below is tests/gat_routes_design.py's arithmetic (float64, index_add only, independent of the
library and of oracle/) with act / act' in place of the clamp and the mask, dout form only; it fills the same fields, so
gat_routes_design's comparisons and metric (errors relative to the ROW's own scale, all-zero rows exactly zero) apply.  The
designed inputs are multiples of 1/4, so z == 0 on about 4 % of the entries: the derivative there is the one torch's
autograd gives (0 relu, slope leaky_relu, alpha elu).

Bound.  D.TOL = 2e-5, the family's.  A float32 torch restatement of the same arithmetic (CPU, `reference(..., dtype=float32)`)
is this far from float64 under the metric, worst quantity, on S o = 16 / B1 o = 32:
    identity 7.8e-7 / 1.0e-6   leaky_relu 7.0e-7 / 1.0e-6   leaky_relu(0.2) 7.0e-7 / 1.0e-6   elu 8.4e-7 / 1.0e-6
    elu(0.5) 8.0e-7 / 1.0e-6   tanh 1.2e-6 / 1.1e-6         sigmoid 1.1e-6 / 1.5e-6
all below D.TOL / 4 = 5e-6, so every activation keeps D.TOL (test_gat_act_abi.py repeats the measurement and asserts it).

The layer tests hold GraphConvolution and MultiHeadGraphConvolution with five activations against oracle.layers_ref.gat_layer
in float64 with gat_layers._gat_forward_general made to raise: the kernel path, not the general one, computed the result.
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
RELU, IDENTITY, LEAKY_RELU, ELU, TANH, SIGMOID = range(6)               # graphode.h: GODE_GAT_ACT_*
# name -> (code, param): every activation of the kernels, leaky_relu and elu at their defaults and at a second parameter
ACTS = {"identity": (IDENTITY, 0.0), "leaky_relu": (LEAKY_RELU, 0.01), "leaky_relu(0.2)": (LEAKY_RELU, 0.2), "elu": (ELU, 1.0),
        "elu(0.5)": (ELU, 0.5), "tanh": (TANH, 0.0), "sigmoid": (SIGMOID, 0.0)}
FAULTS = ("relu_derivative", "alpha_ignored", "forward_only", "zero_from_positive_branch")
PF_LPR = {4: 1, 8: 2, 16: 4, 32: 8, 64: 16}
REC_LPR = {16: 4, 32: 8, 64: 16, 128: 32, 256: 64}
FAMILY = {1: "PF", 2: "WAVE", 3: "GROUP", 4: "REC"}


def act_of(code, p, z):
    """(act(z), act'(z)) in z's dtype; the derivative at z == 0 is torch autograd's."""
    one, pos = torch.ones_like(z), z > 0
    if code == RELU:
        return torch.clamp(z, min=0.0), pos.to(z.dtype)
    if code == IDENTITY:
        return z, one
    if code == LEAKY_RELU:
        return torch.where(pos, z, p * z), torch.where(pos, one, p * one)
    if code == ELU:
        return torch.where(pos, z, p * torch.expm1(z)), torch.where(pos, one, p * torch.exp(z))
    if code == TANH:
        y = torch.tanh(z)
        return y, 1.0 - y * y
    if code == SIGMOID:
        y = 1.0 / (1.0 + torch.exp(-z))
        return y, y * (1.0 - y)
    raise AssertionError(code)


def reference(d, v, act, fault=None, dtype=torch.float64):
    """gat_routes_design.reference with the activation `act` = (code, param), dout form.  fault (one of FAULTS): the same
    arithmetic wrong in one way the kernels could be wrong - relu's derivative (the mask) kept in the backward, the
    parameter ignored (its default used), the activation applied in the forward only (the backward still relu's clamp and
    mask, as when the backward is not told the activation), the derivative at z == 0 taken from the positive branch.
    dtype float32: the same arithmetic in single precision, to measure what fp32 alone costs under the metric."""
    assert fault is None or fault in FAULTS
    code, p = act
    s, t = torch.from_numpy(d.lut[d.src]), torch.from_numpy(d.lut[d.tgt])
    r, c = torch.from_numpy(d.lut[d.rows]), torch.from_numpy(d.cols)
    na, o = v.Ps.shape
    val = torch.ones(d.E, dtype=dtype) if d.vals is None else torch.from_numpy(d.vals).to(dtype)
    a32, amax = D.logits32(d, v)
    w = torch.exp(a32.to(dtype) - amax.to(dtype))
    z = (v.Ps[s] + v.Pt[t]).to(dtype) + v.bf.to(dtype)                         # gathered in fp32 (exact), then converted
    y_fwd, dact = act_of(code, p, z)
    y = y_fwd
    if fault == "relu_derivative":
        dact = (z > 0).to(dtype)
    elif fault == "alpha_ignored":
        y_fwd, dact = act_of(code, {LEAKY_RELU: 0.01, ELU: 1.0}[code], z)
        y = y_fwd
    elif fault == "forward_only":
        y, dact = act_of(RELU, 0.0, z)
    elif fault == "zero_from_positive_branch":
        dact = torch.where(z == 0, torch.ones_like(z), dact)
    we = val * w[c]
    den = torch.zeros(na, dtype=dtype).index_add_(0, r, we) + D.EPS
    out = torch.zeros(na, o, dtype=dtype).index_add_(0, r, we[:, None] * y_fwd[c]) / den[:, None]
    g = v.dout.to(dtype)
    dA = g / den[:, None]
    dsum = -(g * out).sum(1) / den
    dz = torch.zeros(d.E, o, dtype=dtype)
    dz[c] = we[:, None] * dA[r] * dact[c]
    da = torch.zeros(d.E, dtype=dtype)
    da[c] = we * ((dA[r] * y[c]).sum(1) + dsum[r])
    mag = torch.zeros(d.E, dtype=dtype)                                        # da without its cancellation
    mag[c] = we * ((dA[r] * y[c]).abs().sum(1) + dsum[r].abs())
    ref = D.Design()
    ref.a32, ref.amax, ref.w, ref.den, ref.out, ref.dz, ref.da, ref.mag, ref.z = a32, amax, w, den, out, dz, da, mag, z
    ref.share = we / den[r]
    ref.dPs = torch.zeros(na, o, dtype=dtype).index_add_(0, s, dz)
    ref.dPt = torch.zeros(na, o, dtype=dtype).index_add_(0, t, dz)
    ref.dA2 = torch.stack([torch.zeros(na, dtype=dtype).index_add_(0, i, da) for i in (s, t)], 1)
    ref.magA2 = torch.stack([torch.zeros(na, dtype=dtype).index_add_(0, i, mag) for i in (s, t)], 1)
    ref.magPs = torch.zeros(na, o, dtype=dtype).index_add_(0, s, dz.abs())
    ref.magPt = torch.zeros(na, o, dtype=dtype).index_add_(0, t, dz.abs())
    ref.edge_row = torch.empty(d.E, dtype=torch.int64)
    ref.edge_row[c] = r
    return ref


def results_of(ref, got):
    res = dict(D.compare_forward(ref, got.w, got.den, got.out))
    res.update(D.compare_backward(ref, got.dz, got.da, got.dPs, got.dPt, got.dA2))
    return res


@functools.lru_cache(maxsize=None)
def cached_reference(kind, canonical, pattern, o, name):
    return reference(D.design(kind, canonical, pattern), D.values(kind, canonical, o), ACTS[name])


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def code(family, form=0):
    return family | (form << 8)


def maxc(o):
    return 1 if o <= 64 else 2 if o <= 128 else 4 if o <= 256 else 8


def routes():
    import test_gpu_gat_routes as R                                     # its cached designed EdgeGraphs and array helpers
    return R


class Check:
    """Collects every figure of a case, prints it, and fails at the end: one run reports all quantities."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def add(self, route, q, err, exact):
        print("%s %s/%d %-4s err %.3e zero rows exact %s" % (self.case, FAMILY[route & 255], route >> 8, q, err, exact))
        if not (err <= D.TOL and exact):
            self.bad.append((q, err, exact))

    def true(self, cond, what):
        if not cond:
            print("%s FAILED: %s" % (self.case, what))
            self.bad.append(what)

    def done(self):
        assert not self.bad, (self.case, self.bad)


def run_kernels(kind, o, act, canonical=True, pattern=False, split=None, offset=0):
    """Logits, forward, backward (dout form) and the node sums through the ops wrappers with act= `act` (None: the relu entry
    points).  Returns the routes and every output, on the GPU."""
    from graph_odenet_amd import ops
    R = routes()
    d, v = D.design(kind, canonical, pattern), D.values(kind, canonical, o)
    eg = R.edge_graph(kind, canonical, pattern, split)
    n, E = d.n, d.E
    Ps, Pt, A2 = R.full(v.Ps, eg, n), R.full(v.Pt, eg, n), R.full(v.A2, eg, n)
    bf, bw = v.bf.to(dev()), v.bw.to(dev())
    proj = ops.gat_proj(Ps, Pt, A2)
    a, amax = R.sentinel(E), R.sentinel(1)
    ops.gat_logits(proj, bw, eg.src, eg.tgt, a, amax)
    g = D.Design()
    g.eg, g.a, g.amax = eg, a, amax
    g.out, g.w, g.den = R.sentinel(n, o, offset=offset), R.sentinel(E), R.sentinel(n)
    g.fwd_route = ops.gat_agg_fwd_route(eg, proj, o, bf, a, amax, D.EPS, g.out, g.w, g.den, act=act)
    assert g.fwd_route == ops.gat_agg_fwd_route(eg, proj, o, bf, a, amax, D.EPS, g.out, g.w, g.den)   # the relu twin's answer
    ops.gat_agg_fwd(eg, proj, o, bf, a, amax, D.EPS, g.out, g.w, g.den, act=act)
    dout = R.full(v.dout, eg, n)
    g.dz, g.da, g.dPs, g.dPt, g.dA2 = R.sentinel(E, o), R.sentinel(E), R.sentinel(n, o), R.sentinel(n, o), R.sentinel(n, 2)
    kw = dict(dPt=g.dPt, dA2=g.dA2, dout=dout)
    g.bwd_route = ops.gat_agg_bwd_route(eg, proj, o, bf, g.w, g.den, g.out, g.dz, g.da, act=act, **kw)
    assert g.bwd_route == ops.gat_agg_bwd_route(eg, proj, o, bf, g.w, g.den, g.out, g.dz, g.da, **kw)
    g.did = ops.gat_agg_bwd(eg, proj, o, bf, g.w, g.den, g.out, g.dz, g.da, act=act, **kw)
    assert g.did == ((g.bwd_route & 255) == 4), ("did_target_sums", g.did, g.bwd_route)
    g.target_sums = (g.dPt.clone(), g.dA2.clone())                         # as the aggregation's backward left them
    if g.did:                                                              # the source side is two incidence products
        ops.spmm(eg.Ms_inc, g.dz, out=g.dPs)
        ops.spmm(eg.Ms_inc, g.da.view(-1, 1), out=g.dA2[:, 0:1])
    else:
        ops.gat_scatter(eg.Ms_inc, eg.Mt_inc, g.dz, g.da, g.dPs, g.dPt, g.dA2)
    return g


def run_case(kind, o, name, fwd_route, bwd_route, canonical=True, pattern=False, split=None, offset=0):
    d = D.design(kind, canonical, pattern)
    case = "%s %s%s%s o=%d" % (name, kind, "" if canonical else " non-canonical", " pattern" if pattern else "", o)
    g = run_kernels(kind, o, ACTS[name], canonical, pattern, split, offset)
    assert g.fwd_route == fwd_route, (case, "forward route", g.fwd_route, fwd_route)
    assert g.bwd_route == bwd_route, (case, "backward route", g.bwd_route, bwd_route)
    ref = cached_reference(kind, canonical, pattern, o, name)
    eg, ck = g.eg, Check(case)
    ck.true(torch.equal(g.a.cpu(), ref.a32) and g.amax.item() == ref.amax.item(), "logits bit for bit")
    for q, res in D.compare_forward(ref, g.w.cpu(), g.den[eg.act].cpu(), g.out[eg.act].cpu()).items():
        ck.add(g.fwd_route, q, *res)
    ck.true(bool((g.out[eg.inactive] == 0).all()) and bool((g.den[eg.inactive] == np.float32(D.EPS)).all()),
            "rows without edges: out 0, den eps")
    if not g.did:
        ck.true(bool((g.target_sums[0] == SENT).all()) and bool((g.target_sums[1] == SENT).all()),
                "dPt / dA2 untouched off the record route")
    for q, res in D.compare_backward(ref, g.dz.cpu(), g.da.cpu(), g.dPs[eg.act].cpu(), g.dPt[eg.act].cpu(), g.dA2[eg.act].cpu()).items():
        ck.add(g.bwd_route, q, *res)
    ck.true(all(bool((x[eg.inactive] == 0).all()) for x in (g.dPs, g.dPt, g.dA2)), "node sums of rows without edges are 0")
    ck.true(0.03 < (ref.z == 0).double().mean().item() < 0.06 and d.E > 0, "z == 0 occurs in the designed inputs")
    ck.done()


@gpu
@pytest.mark.parametrize("name", list(ACTS))
def test_every_activation_on_the_prefetched_route(name):
    run_case("S", 16, name, code(1, 4), code(1, 4))


@gpu
@pytest.mark.parametrize("name", list(ACTS))
def test_every_activation_on_the_record_route(name):
    """65 537 busy rows, o = 32, rows split at 96 (the finishing launches do not depend on the activation)."""
    run_case("B1", 32, name, code(4, 8), code(4, 8), split=D.SPLIT)


@gpu
def test_elu_prefetched_four_rows_per_wave():
    run_case("S", 4, "elu", code(1, 1), code(1, 1))


@gpu
@pytest.mark.parametrize("o", [73, 200])
def test_elu_wave_route(o):
    run_case("S", o, "elu", code(2, maxc(o)), code(2, maxc(o)))


@gpu
def test_elu_wave_route_as_the_unaligned_fallback():
    run_case("S", 16, "elu", code(2, 1), code(2, 1), offset=1)


@gpu
def test_elu_group_route():
    run_case("B1", 24, "elu", code(3, 1), code(3, 1))


@gpu
def test_elu_record_route_with_split_rows():
    run_case("L", 64, "elu", code(4, 16), code(4, 16), split=D.SPLIT)


@gpu
@pytest.mark.parametrize("kind,o,family", [("S", 8, 1), ("S", 73, 2), ("L", 16, 3)])
def test_elu_non_canonical_mtgt(kind, o, family):
    """Mtgt rows that disagree with tgt: an edge's Pt row is not its row's, and `col` keeps the record route away."""
    rt = code(family, PF_LPR[o] if family == 1 else maxc(o))
    run_case(kind, o, "elu", rt, rt, canonical=False)


@gpu
@pytest.mark.parametrize("kind,o,split,family", [("S", 16, None, 1), ("L", 32, D.SPLIT, 4)])
def test_elu_pattern_only_mtgt(kind, o, split, family):
    rt = code(family, PF_LPR[o] if family == 1 else REC_LPR[o])
    run_case(kind, o, "elu", rt, rt, pattern=True, split=split)


@gpu
@pytest.mark.parametrize("kind,o,split,rt", [("S", 16, None, code(1, 4)), ("B1", 32, D.SPLIT, code(4, 8))])
def test_relu_through_the_new_entry_points_is_the_old_entry_points(kind, o, split, rt):
    old = run_kernels(kind, o, None, split=split)
    new = run_kernels(kind, o, (RELU, 0.0), split=split)
    assert old.fwd_route == new.fwd_route == rt and old.bwd_route == new.bwd_route == rt and old.did == new.did
    for q in ("out", "w", "den", "dz", "da", "dPs", "dPt", "dA2"):
        assert torch.equal(getattr(old, q), getattr(new, q)), q
    assert torch.equal(old.target_sums[0], new.target_sums[0]) and torch.equal(old.target_sums[1], new.target_sums[1])
    ref = D.reference(D.design(kind), D.values(kind, True, o))            # and both are the relu restatement's
    eg = old.eg
    assert D.passes(D.compare_forward(ref, new.w.cpu(), new.den[eg.act].cpu(), new.out[eg.act].cpu()))


# ---- the layers -----------------------------------------------------------------------------------------------------------
def layer_acts():
    import torch.nn as nn
    import torch.nn.functional as F
    return {"elu": F.elu, "leaky_relu(0.2)": nn.LeakyReLU(0.2), "tanh": torch.tanh, "sigmoid": nn.Sigmoid(), "identity": nn.Identity()}


def layer_inputs(H, E=1900):
    g = torch.Generator().manual_seed(31 + H)
    n, nin, o = 211, 9, 6
    src, tgt = torch.randint(0, n, (E,), generator=g), torch.randint(0, n - 3, (E,), generator=g)
    Mtgt = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(E)]), torch.ones(E), (n, E))
    x, gout = torch.randn(n, nin, generator=g), torch.randn(n, H * o, generator=g)
    return n, nin, o, src, tgt, Mtgt, x, gout


def make_layer(H, nin, o, act):
    from graph_odenet_amd.gat_heads import MultiHeadGraphConvolution
    from graph_odenet_amd.gat_layers import GraphConvolution
    torch.manual_seed(H)
    layer = GraphConvolution(nin, o, act=act) if H == 1 else MultiHeadGraphConvolution(nin, H * o, heads=H, act=act)
    return layer, ([layer] if H == 1 else list(layer.heads))


def general_path_must_not_run(*a, **k):
    raise AssertionError("the general path ran for an activation the kernels restate")


@gpu
@pytest.mark.parametrize("act_name", ["elu", "leaky_relu(0.2)", "tanh", "sigmoid", "identity"])
@pytest.mark.parametrize("H", [1, 4])
def test_layers_take_the_kernel_path_vs_fp64_oracle(act_name, H, monkeypatch):
    """n = 211, E = 1 900 (the graph of test_gpu_gat_heads.test_non_relu_activation_vs_fp64_oracle), output and every gradient
    against the fp64 oracle at that test's 1e-5 / 2e-5, with the general path made to raise."""
    from graph_odenet_amd import gat_layers
    from oracle import layers_ref as R
    from test_gpu_gat_heads import close
    monkeypatch.setattr(gat_layers, "_gat_forward_general", general_path_must_not_run)
    act = layer_acts()[act_name]
    n, nin, o, src, tgt, Mtgt, x, gout = layer_inputs(H)
    layer, hds = make_layer(H, nin, o, act)
    xd = x.double().requires_grad_(True)
    ps = [[p.detach().double().requires_grad_(True) for p in (hd.f.weight, hd.f.bias, hd.w.weight, hd.w.bias)] for hd in hds]
    ref = torch.cat([R.gat_layer(xd, src, tgt, Mtgt.double(), *p4, act=act) for p4 in ps], 1)
    ref.backward(gout.double())
    layer = layer.to(dev())
    xg = x.to(dev()).requires_grad_(True)
    out = layer(xg, src.to(dev()), tgt.to(dev()), Mtgt.to(dev()))
    close(out, ref, 1e-5, "out")
    out.backward(gout.to(dev()))
    close(xg.grad, xd.grad, 2e-5, "gx")
    for hd, p4 in zip(hds, ps):
        for p, q in zip((hd.f.weight, hd.f.bias, hd.w.weight, hd.w.bias), p4):
            close(p.grad, q.grad, 2e-5, "param")


@gpu
@pytest.mark.parametrize("H", [1, 4])
def test_a_lambda_still_takes_the_general_path_once_per_head(H, monkeypatch):
    import torch.nn.functional as F
    from graph_odenet_amd import gat_layers
    calls, general = [], gat_layers._gat_forward_general

    def counting(*a, **k):
        calls.append(1)
        return general(*a, **k)

    monkeypatch.setattr(gat_layers, "_gat_forward_general", counting)
    n, nin, o, src, tgt, Mtgt, x, gout = layer_inputs(H)
    layer, _ = make_layer(H, nin, o, lambda v: F.elu(v))
    out = layer.to(dev())(x.to(dev()), src.to(dev()), tgt.to(dev()), Mtgt.to(dev()))
    assert len(calls) == H and out.shape == (n, H * o)


@gpu
@pytest.mark.parametrize("H", [1, 4])
def test_no_edges_gives_zeros_with_a_grad_fn(H, monkeypatch):
    import torch.nn.functional as F
    from graph_odenet_amd import gat_layers
    monkeypatch.setattr(gat_layers, "_gat_forward_general", general_path_must_not_run)
    n, nin, o, src, tgt, Mtgt, x, gout = layer_inputs(H, E=0)
    layer, hds = make_layer(H, nin, o, F.elu)
    layer = layer.to(dev())
    xg = x.to(dev()).requires_grad_(True)
    out = layer(xg, src.to(dev()), tgt.to(dev()), Mtgt.to(dev()))
    assert out.shape == (n, H * o) and bool((out == 0).all()) and out.grad_fn is not None
    out.backward(gout.to(dev()))
    assert bool((xg.grad == 0).all()) and all(p.grad is None or bool((p.grad == 0).all()) for p in layer.parameters())
