"""H-head edge attention (BASELINE.json configs[2]: "Citeseer GAT 8-head ODEBlock rk4"; SURVEY.md §8(d) C3: "8
independent reference-style heads batched").  The reference's layer (GAT/layers.py:11-63) has one head; an H-head
layer here is H of those layers on the same graph with their outputs concatenated,

    out = [ head_0(x) | head_1(x) | ... | head_{H-1}(x) ]          head_h : in_features -> out_features / H,

each head with its own f / w Linear layers, its own global logit maximum (:47) and its own eps-regularised
per-target normalisation (:53) - the parameters are literally H reference layers (`heads.<h>.f.weight`, ...).

Execution: the H heads run as ONE head on the H-fold graph.  Virtual node v*H + h carries head h of node v, so the
N x (H*o) projection matrices of all heads - produced by ONE dense product with the heads' weights side by side,
square (d+1) x d inside an ODE function where H*o = d - ARE the (N*H) x o matrices of the virtual nodes, and the
(N*H) x o result is the N x (H*o) concatenation: no copy in either direction.  Edge s -> t becomes the H edges
s*H+h -> t*H+h.  Every aggregation / VJP / scatter kernel of the one-head path runs unchanged on that graph; the
per-head maximum is handled by gode_gat_logits_heads_f32 (logits shifted by their head's maximum, the aggregation then
runs with amax = 0) and gode_gat_maxpath_heads_f32 (gradient path through each head's maximum).  The per-head message
biases are folded into the target-side projection (z_e = Ps[src] + (Pt[tgt] + bf_h)); the logit biases are added by the
logits kernel.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.modules.module import Module

from . import ops
from . import models as _gcn_models
from .gat_layers import EdgeGraph, GraphConvolution, _kernel_act, edge_graph, message_activation
from .gat_ode import gat_fields
from .models import _gn


def heads_graph(eg, heads):
    """The H-fold EdgeGraph of `eg` (cached on it)."""
    cache = eg.__dict__.setdefault("_heads", {})
    hit = cache.get(heads)
    if hit is not None:
        return hit
    if not eg.canonical:
        raise NotImplementedError("multi-head attention needs an Mtgt whose rows agree with tgt")
    dev = eg.src.device
    h = torch.arange(heads, device=dev)
    src_v = (eg.src.to(torch.int64)[:, None] * heads + h).reshape(-1)
    tgt_v = (eg.tgt.to(torch.int64)[:, None] * heads + h).reshape(-1)
    ev = eg.E * heads
    val = eg.Mt.val.repeat_interleave(heads) if eg.Mt.val is not None else torch.ones(ev, device=dev)
    M = torch.sparse_coo_tensor(torch.stack([tgt_v, torch.arange(ev, device=dev)]), val, (eg.n * heads, ev))
    egv = EdgeGraph(src_v, tgt_v, M)
    if not egv.canonical:
        raise RuntimeError("H-fold graph lost its target order")
    egv.base, egv.heads = eg, heads
    cache[heads] = egv
    return egv


class _EdgeAttentionHeadsFn(torch.autograd.Function):
    """Concatenated outputs of H heads from Ps, Pt (N x H*o, biases folded into Pt) and A2 (N x 2H: per head the
    logit part by source and by target, bias folded into the latter)."""

    @staticmethod
    def forward(ctx, egv, heads, Ps, Pt, A2, eps, act=None):
        Ps, Pt, A2 = Ps.contiguous(), Pt.contiguous(), A2.contiguous()
        n, d = Ps.shape
        o, nv = d // heads, n * heads
        f = dict(dtype=torch.float32, device=Ps.device)
        a, zero = torch.empty(egv.E, **f), torch.zeros(1, **f)
        out, w, den = torch.empty(n, d, **f), torch.empty(egv.E, **f), torch.empty(nv, **f)
        proj = ops.gat_proj(Ps.view(nv, o), Pt.view(nv, o), A2.view(nv, 2))
        ops.gat_logits_heads(proj, egv.src, egv.tgt, heads, a)
        ops.gat_agg_fwd(egv, proj, o, torch.zeros(o, **f), a, zero, eps, out.view(nv, o), w, den, act=act)
        ctx.egv, ctx.heads, ctx.act = egv, heads, act
        ctx.save_for_backward(Ps, Pt, A2, a, w, den, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        Ps, Pt, A2, a, w, den, out = ctx.saved_tensors
        egv, heads = ctx.egv, ctx.heads
        n, d = Ps.shape
        o, nv = d // heads, n * heads
        f = dict(dtype=torch.float32, device=Ps.device)
        dz, da = torch.empty(egv.E, o, **f), torch.empty(egv.E, **f)
        dPs, dPt, dA2 = torch.empty(n, d, **f), torch.empty(n, d, **f), torch.empty(n, 2 * heads, **f)
        proj = ops.gat_proj(Ps.view(nv, o), Pt.view(nv, o), A2.view(nv, 2))
        ops.gat_vjp(egv, proj, o, torch.zeros(o, **f), a, torch.zeros(1, **f), w, den, out.view(nv, o), dz, da,
                    dPs.view(nv, o), dPt.view(nv, o), dA2.view(nv, 2), dout=dout.contiguous().view(nv, o), heads=heads,
                    act=ctx.act)
        return None, None, dPs, dPt, dA2, None, None


class MultiHeadGraphConvolution(Module):
    """`heads` reference layers (GAT/layers.py:11-63) on one graph, outputs concatenated."""

    def __init__(self, in_features, out_features, heads=8, bias=True, act=F.relu, eps=1e-6):
        super(MultiHeadGraphConvolution, self).__init__()
        if heads < 1 or out_features % heads:
            raise ValueError("MultiHeadGraphConvolution: %d heads do not divide %d output features" % (heads, out_features))
        if heads > 64:
            raise ValueError("MultiHeadGraphConvolution: at most 64 heads")
        self.in_features, self.out_features, self.n_heads = in_features, out_features, heads
        self.eps, self.act = eps, act
        self.heads = nn.ModuleList([GraphConvolution(in_features, out_features // heads, bias, act, eps)
                                    for _ in range(heads)])

    def packed(self):
        """(Wsrc, Wtgt: i x H*o;  Wlog: i x 2H;  bf: H*o;  ba: 2H = [0, bw_0, 0, bw_1, ...]) as differentiable
        functions of the heads' parameters."""
        # a handful of launches whatever the head count (one stack per parameter kind, one permuted copy per block): the
        # per-head cat / stack / zeros_like form cost ~30 launches per call and ~150 per training step at 8 heads
        i, H, o = self.in_features, self.n_heads, self.out_features // self.n_heads
        Wf = torch.stack([hd.f.weight for hd in self.heads])                    # H x o x 2i
        Wsrc = Wf[:, :, :i].permute(2, 0, 1).reshape(i, H * o)
        Wtgt = Wf[:, :, i:].permute(2, 0, 1).reshape(i, H * o)
        ww = torch.stack([hd.w.weight[0] for hd in self.heads])                 # H x 2i
        Wlog = ww.view(H, 2, i).permute(2, 0, 1).reshape(i, 2 * H)              # column 2h: source part, 2h+1: target part
        bf = torch.cat([hd.f.bias for hd in self.heads])
        bw = torch.cat([hd.w.bias for hd in self.heads])
        ba = torch.stack([torch.zeros_like(bw), bw], 1).reshape(2 * H)
        return Wsrc, Wtgt, Wlog, bf, ba

    def forward(self, x, src, tgt, Mtgt):
        return _heads_forward(self, x, src, tgt, Mtgt)

    def __repr__(self):
        return "%s (%d -> %d, %d heads)" % (self.__class__.__name__, self.in_features, self.out_features, self.n_heads)


def _heads_forward(layer, x, src, tgt, Mtgt):
    ka = _kernel_act(layer)
    if ka is False:                      # an activation the kernels do not restate: every head through the general (unfused) layer path
        return torch.cat([hd(x, src, tgt, Mtgt) for hd in layer.heads], 1)
    eg = edge_graph(src, tgt, Mtgt)
    if not eg.canonical and layer.act is not F.relu:  # no H-fold graph of such an Mtgt: every head through the one-head kernels
        return torch.cat([hd(x, src, tgt, Mtgt) for hd in layer.heads], 1)
    Wsrc, Wtgt, Wlog, bf, ba = layer.packed()
    from .functional import dense
    Ps, Pt, A2 = dense(x, Wsrc), dense(x, Wtgt, bf), dense(x, Wlog, ba)
    if eg.E == 0:
        return torch.zeros(x.shape[0], layer.out_features, dtype=x.dtype, device=x.device) + 0.0 * (Ps.sum() + Pt.sum() + A2.sum())
    return _EdgeAttentionHeadsFn.apply(heads_graph(eg, layer.n_heads), layer.n_heads, Ps, Pt, A2, layer.eps, ka)


class FixedMultiHeadGraphConvolution(MultiHeadGraphConvolution):
    """The same layer with (src, tgt, Mtgt) held as attributes (the role of GAT/layers.py:67-127)."""

    def __init__(self, in_features, out_features, heads=8, bias=True, act=F.relu, eps=1e-6):
        super(FixedMultiHeadGraphConvolution, self).__init__(in_features, out_features, heads, bias, act, eps)
        self.src = self.tgt = self.Mtgt = torch.Tensor([[1]])

    def set_adj(self, src, tgt, Mtgt):
        self.src, self.tgt, self.Mtgt = src, tgt, Mtgt

    def forward(self, x):
        return _heads_forward(self, x, self.src, self.tgt, self.Mtgt)


class ODEfunc(nn.Module):
    """relu(gc1([t | norm1(x)])) with an H-head layer: GAT/models.py:161-179 with `heads` reference layers side by
    side (dim must be a multiple of heads).  act: the message activation of every head (gc1.act is the one that counts)."""

    _gode_counts_nfe = True

    def __init__(self, dim, heads=8, act=F.relu):
        super(ODEfunc, self).__init__()
        self.norm1 = _gn(dim)
        self.gc1 = FixedMultiHeadGraphConvolution(dim + 1, dim, heads, act=act)
        self.nfe = 0

    def set_adj(self, src, tgt, Mtgt):
        self.gc1.set_adj(src, tgt, Mtgt)

    def forward(self, t, x):
        self.nfe += 1
        xn = self.norm1(x)
        return F.relu(self.gc1(torch.cat([torch.ones_like(xn[:, :1]) * t, xn], 1)))

    def _egv(self):
        layer = self.gc1
        if not torch.is_tensor(layer.src) or layer.src.dim() != 1:
            return None
        eg = edge_graph(layer.src, layer.tgt, layer.Mtgt)
        return heads_graph(eg, layer.n_heads) if eg.canonical and eg.E > 0 else None

    def gode_plan_token(self, y0):
        egv = self._egv()
        # the activation's (code, param) are kernel arguments of a captured solve: a changed gc1.act is another plan
        return None if egv is None else ("gat-heads", id(egv), message_activation(self.gc1.act))

    def gode_fields(self, y0):
        """Hook for graph_odenet_amd.odeint: fused forward / adjoint kernel sequences (gat_ode.py)."""
        layer, norm = self.gc1, self.norm1
        egv = self._egv()
        if egv is None:
            return None
        names = {id(norm.weight): "gamma", id(norm.bias): "beta"}
        if layer.n_heads == 1:           # the reference's layer: the one-head sequence on the base graph
            hd = layer.heads[0]
            names.update({id(hd.f.weight): "Wf", id(hd.f.bias): "bf", id(hd.w.weight): "ww", id(hd.w.bias): "bw"})
            return gat_fields(self, hd, egv.base, egv.base.n, names, y0, act_layer=layer)
        for h, hd in enumerate(layer.heads):
            names.update({id(hd.f.weight): "Wf%d" % h, id(hd.f.bias): "bf%d" % h, id(hd.w.weight): "ww%d" % h,
                          id(hd.w.bias): "bw%d" % h})
        return gat_fields(self, layer, egv, egv.base.n, names, y0)


class ODEfunc2(nn.Module):
    """Two stacked (H-head layer -> relu -> GroupNorm) with the time column re-attached before each layer: the GAT
    variant's ODEfunc2 (GAT/models.py:551-575) with `heads` reference layers side by side in both positions."""

    def __init__(self, dim, dropout, heads=8):
        super(ODEfunc2, self).__init__()
        self.norm1, self.norm2 = _gn(dim), _gn(dim)
        self.gc1 = FixedMultiHeadGraphConvolution(dim + 1, dim, heads)
        self.gc2 = FixedMultiHeadGraphConvolution(dim + 1, dim, heads)
        self.dropout = dropout
        self.nfe = 0

    def set_adj(self, src, tgt, Mtgt):
        self.gc1.set_adj(src, tgt, Mtgt)
        self.gc2.set_adj(src, tgt, Mtgt)

    def forward(self, t, x):
        self.nfe += 1
        tt = torch.ones_like(x[:, :1]) * t
        x = self.norm1(F.relu(self.gc1(torch.cat([tt, x], 1))))
        return self.norm2(F.relu(self.gc2(torch.cat([tt, x], 1))))


# ---- model zoo ----------------------------------------------------------------------------------------------------
_zoos = {}
MIN_HEAD_WIDTH = 4


def zoo(heads=8):
    """The 23 model classes of the GAT variant with H-head layers wherever `heads` divides the layer's output width
    into heads of at least MIN_HEAD_WIDTH features (the hidden layers and the ODE block; a class-count output layer
    keeps one head, as in the usual GAT output layer).  Returns a namespace object with the classes as attributes."""
    hit = _zoos.get(heads)
    if hit is not None:
        return hit

    def layer(in_features, out_features, *args, **kw):
        if out_features % heads == 0 and out_features // heads >= MIN_HEAD_WIDTH:
            return MultiHeadGraphConvolution(in_features, out_features, heads, *args, **kw)
        return GraphConvolution(in_features, out_features, *args, **kw)

    def odefunc(dim):
        return ODEfunc(dim, heads)

    def odefunc2(dim, dropout):
        return ODEfunc2(dim, dropout, heads)

    kit = type("GatHeadsKit%d" % heads, (), {"GraphConvolution": staticmethod(layer), "ODEfunc": staticmethod(odefunc),
                                             "ODEfunc2": staticmethod(odefunc2), "input_dropout": False})

    def _forward(self, x, src, tgt, Mtgt):
        return self._body(self._input(x), (src, tgt, Mtgt))

    ns = {}
    _gcn_models.rebind_zoo(ns, __name__, kit, forward=_forward, what="%d-head GAT" % heads)
    out = _zoos[heads] = type("GatHeadsZoo%d" % heads, (), ns)
    return out
