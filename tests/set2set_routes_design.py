"""Designed inputs and the float64 restatement for the Set2Set readout route tests (test_set2set_routes.py checks the
design's conditions on the CPU, test_gpu_set2set_routes.py runs the kernels on it).  numpy / CPU torch only; nothing of the
library and nothing of oracle/ is used here.

Three kernel families are covered: the one-launch readout loop (csrc/set2set.hip), the fused LSTM cell of the per-step
path (csrc/lstm.hip) and the per-graph softmax readout (csrc/segment.hip).  The limits their routes branch on are written
out below as plain numbers; every case carries the route it is meant to reach, stated from those numbers, and
test_set2set_routes.py recomputes it.

Inputs.  LSTM weights are drawn as nn.LSTM draws them, U(-1/sqrt(H), 1/sqrt(H)); x is N(0, 1) (times `xscale`), the
cotangent on the final q* is N(0, 1).  Every batch of the loop's width table holds graphs of 1, 0, 2, 15, 16, 17 and 33
nodes (one trip of the loop kernel's 16 waves, bracketed), one graph of exactly 12288 // H nodes (the largest whose rows are
staged in LDS) and one of 12288 // H + 1 (the smallest that is not).

Conditioning.  Two cases are reseeded (`reseed`), on the evidence of the float32 restatement alone: with x scaled by 30 the
second step's gate pre-activations and the attention's backward (terms of size 30^2 that cancel) leave plain float32
arithmetic between 4e-6 and 3e-4 away from float64 on the parameter gradients, depending on the draw (8 seeds tried), and
at H = 257, T = 12 between 1.2e-6 and 4.6e-6 on the gradients.  The draws kept are the ones where float32 itself stays a factor 4
inside the tolerances; test_set2set_routes.py asserts that for every case.
"""
import functools
import math

import numpy as np
import torch

# ---- the limits the routes branch on -------------------------------------------------------------------------------------
NT = 1024                 # csrc/set2set.hip `NT`: threads per workgroup of the loop kernels
LANES = 64                # a wave; the feature chunk of the loop's and the segment kernels' lanes
WAVES = NT // LANES       # csrc/set2set.hip `kWaves` = 16: a graph's nodes are strided over the waves
XCAP = 12288              # csrc/set2set.hip `kXCap`: floats of LDS for a graph's node rows; nb * H above it -> un-staged
S2S_HMAX = 512            # csrc/set2set.hip gode_set2set_supported
S2S_STEPS_MAX = 4096      # csrc/set2set.hip gode_set2set_f32_fwd/_bwd: more steps -> GODE_E_RANGE
SEG_HMAX = 1024           # csrc/segment.hip gode_segment_attention_f32_fwd/_bwd: wider -> GODE_E_UNSUPPORTED
SEG_THREADS = 256         # csrc/segment.hip: 4 waves; the rescale loop advances by 256 nodes
SEG_MCS = (1, 2, 4, 8, 16)   # csrc/segment.hip GODE_SEG_DISPATCH: instantiated chunks of 64 columns per lane
LSTM_LDS = 24576          # csrc/lstm.hip `kLstmMaxLds`: floats of LDS a launch may ask for
LSTM_ROWS = 64            # csrc/lstm.hip gode_lstm_cell_f32_fwd: rows of [x | h] per chunk, at most one wave's lanes
E_NULLPTR, E_SHAPE, E_RANGE, E_UNSUPPORTED = -1, -2, -4, -5      # include/graphode.h

TOL_FWD, TOL_GRAD = 1e-5, 2e-5          # the loop and the segment attention (test_set2set_module_vs_reference_golden)
TOL_CAP = 1e-4                          # large-logit cases: max(tolerance, 4 x e32), never above this
LSTM_TOL_FWD, LSTM_TOL_GRAD = 2e-6, 4e-6   # the LSTM cell (test_fused_lstm_cell_vs_float64); the latter times sqrt(B)

FWD_KEYS = ("qs", "cs", "gates", "att")
GRAD_KEYS = ("dx", "dw_ih", "dw_hh", "db_ih", "db_hh")


# ---- routes, from the numbers above --------------------------------------------------------------------------------------
def matvec_route(nj):
    """matvec_cols with nj outputs: (threads per k slice, k slices, passes, outputs of the last pass, idle threads)."""
    jp = -(-nj // LANES) * LANES if nj < NT else NT
    ks = max(NT // jp, 1)
    passes = -(-nj // jp)
    return jp, ks, passes, nj - (passes - 1) * jp, NT - ks * jp


def loop_route(H, sizes, sorted_batch):
    """The tags of the routes a loop case reaches."""
    tags = {"sorted" if sorted_batch else "unsorted"}
    jp, ks, passes, last, idle = matvec_route(4 * H)
    tags.add("passes%d" % passes)
    tags.add("kslices%d" % ks)
    if idle:
        tags.add("idle_threads")
    if passes > 1 and last < jp:
        tags.add("partial_last_pass")
    if 4 * H == NT:
        tags.add("4H==NT")
    if 2 * H == NT:
        tags.add("2H==NT")
    for nb in sizes:
        tags.add("staged" if nb * H <= XCAP else "unstaged")
        if nb > NT:
            tags.add("over1024")
        if nb == 0:
            tags.add("empty")
        if nb > WAVES:
            tags.add("wave_trips>1")
    if sizes[0] * H > XCAP and sizes[-1] * H > XCAP:
        tags.add("unstaged_first_last")
    if len(sizes) == 1:
        tags.add("one_graph")
    return tags


def seg_mc(h):
    """The instantiation GODE_SEG_DISPATCH picks: the first of 1, 2, 4, 8, 16 that holds ceil(h / 64) chunks."""
    need = -(-h // LANES)
    return next(m for m in SEG_MCS if need <= m)


def lstm_supported(B, I, H):
    """gode_lstm_cell_supported, from the LDS budget: backward B x (4H + 1) + 4B + 16H floats, forward 6 (I + H) + 256."""
    return B > 0 and I > 0 and H > 0 and B * (4 * H + 1) + 4 * B + 16 * H <= LSTM_LDS and 6 * (I + H) + 256 <= LSTM_LDS


def lstm_chunks(B, I, H):
    """(rows per chunk, chunks, whether LDS and not the 64 lanes or B limits the chunk) of the forward cell."""
    K = I + H
    by_lds = (LSTM_LDS - 256 - 4 * K) // (K | 1)
    cb = min(by_lds, LSTM_ROWS, B)
    return cb, -(-B // cb), by_lds < min(LSTM_ROWS, B)


def set2set_supported(H):
    return 0 < H <= S2S_HMAX


# ---- case tables ---------------------------------------------------------------------------------------------------------
class LoopCase:
    def __init__(self, name, H, T=3, sizes=None, sorted_batch=True, bias=True, xscale=1.0, strided=False, reaches=(), reseed=0):
        self.name, self.H, self.T, self.sorted_batch, self.bias, self.xscale, self.strided = name, H, T, sorted_batch, bias, xscale, strided
        self.sizes = list(sizes) if sizes is not None else width_sizes(H)
        self.reaches = set(reaches)            # the routes the case is meant for; test_set2set_routes.py recomputes them
        self.seed = 1000 + 7 * H + 31 * T + 3 * len(self.sizes) + (0 if sorted_batch else 1) + (0 if bias else 2) + (5 if strided else 0) + reseed
        self.large_logits = xscale != 1.0

    def __repr__(self):
        return self.name


def width_sizes(H):
    return [1, 0, 2, 15, 16, 17, 33, XCAP // H, XCAP // H + 1]


WIDTHS = (1, 3, 16, 63, 64, 65, 73, 128, 129, 255, 256, 257, 300, 511, 512)
_WIDTH_REACHES = {
    1: {"kslices16", "over1024"}, 3: {"kslices16", "over1024"}, 16: {"kslices16"}, 63: {"kslices4"}, 64: {"kslices4"}, 65: {"kslices3"},
    73: {"kslices3", "idle_threads"}, 128: {"kslices2"}, 129: {"kslices1", "idle_threads"}, 255: {"kslices1", "passes1"},
    256: {"4H==NT", "passes1", "kslices1"}, 257: {"passes2", "partial_last_pass"}, 300: {"passes2", "partial_last_pass"},
    511: {"passes2", "partial_last_pass"}, 512: {"passes2", "2H==NT"}}
_BOTH = {"staged", "unstaged", "empty", "wave_trips>1"}

LOOP_CASES = [LoopCase("width%d" % H, H, reaches=_BOTH | _WIDTH_REACHES[H] | {"sorted"}) for H in WIDTHS]
LOOP_CASES += [LoopCase("steps%d_h%d" % (T, H), H, T=T, reaches=_BOTH | {"sorted"}, reseed=400 if (T, H) == (12, 257) else 0)
               for H in (73, 257) for T in (1, 2, 12)]
LOOP_CASES += [LoopCase("unsorted_h%d" % H, H, sorted_batch=False, reaches=_BOTH | {"unsorted"} | r)
               for H, r in ((16, {"passes1"}), (73, {"passes1"}), (256, {"4H==NT"}), (257, {"passes2"}), (512, {"passes2", "2H==NT"}))]
LOOP_CASES += [LoopCase("nobias_h%d" % H, H, bias=False, reaches=_BOTH) for H in (73, 300)]
LOOP_CASES += [LoopCase("n1100_h%d_%s" % (H, "sorted" if s else "unsorted"), H, sizes=[3, 1100, 0, 5], sorted_batch=s,
                        reaches={"over1024", route, "sorted" if s else "unsorted"})
               for H, route in ((8, "staged"), (16, "unstaged")) for s in (True, False)]
LOOP_CASES += [LoopCase("one_graph", 73, sizes=[37], reaches={"one_graph", "staged"}),
               LoopCase("unstaged_ends", 73, sizes=[XCAP // 73 + 1, 5, 0, 20, XCAP // 73 + 2], reaches={"unstaged_first_last"}),
               LoopCase("large_logits", 73, T=2, xscale=30.0, reaches=_BOTH, reseed=400),
               LoopCase("strided_h73", 73, strided=True, reaches=_BOTH | {"sorted"}),
               LoopCase("strided_h16", 16, strided=True, sorted_batch=False, reaches=_BOTH | {"unsorted"})]
LOOP_BY_NAME = {c.name: c for c in LOOP_CASES}
assert len(LOOP_BY_NAME) == len(LOOP_CASES)

# (B, I, H) -> what it reaches
LSTM_CASES = [((65, 32, 16), "2 chunks"), ((128, 32, 16), "2 chunks"), ((130, 32, 16), "3 chunks"),
              ((20, 3000, 8), "lds-limited"), ((78, 146, 73), "largest B"), ((1, 1, 1), "1 chunk")]

SEG_WIDTHS = (1, 63, 64, 65, 128, 129, 256, 257, 300, 512, 513, 1023)
SEG_SIZES = [1, 40, 0, 7, 23, 2, 64, 5, 255, 256, 257, 1000]


class SegCase:
    def __init__(self, name, h, sorted_batch=True, qscale=1.0, strided=False):
        self.name, self.h, self.sorted_batch, self.qscale, self.strided = name, h, sorted_batch, qscale, strided
        self.sizes = SEG_SIZES
        self.mc = seg_mc(h)
        self.large_logits = qscale != 1.0
        self.seed = 500 + 3 * h + (0 if sorted_batch else 1) + (7 if strided else 0)

    def __repr__(self):
        return self.name


SEG_CASES = [SegCase("h%d_%s" % (h, "sorted" if s else "unsorted"), h, s) for h in SEG_WIDTHS for s in (True, False)]
SEG_CASES += [SegCase("large_logits", 73, True, qscale=40.0), SegCase("strided_h73", 73, False, strided=True)]
SEG_BY_NAME = {c.name: c for c in SEG_CASES}

MODULE_CASES = [(513, "per-step"), (512, "one-launch")]          # Set2Set(in_channels, 3)
MODULE_SIZES = [1, 0, 2, 17, 33, XCAP // 512, XCAP // 512 + 1]   # 7 graphs: the most the LSTM cell takes at H = 513
PAD = 3                                                          # strided cases: x is columns 1 .. H of an N x (H + 3) matrix


# ---- inputs --------------------------------------------------------------------------------------------------------------
class Bag:
    pass


def batch_vector(sizes, sorted_batch, rs):
    batch = np.repeat(np.arange(len(sizes)), sizes)
    if not sorted_batch:
        batch = batch[rs.permutation(batch.size)]
    return torch.from_numpy(batch.astype(np.int64))


def position_in_graph(batch):
    """Rank of every node among the nodes of its graph in ascending node order (the order of the kernels' segments)."""
    b = batch.numpy()
    order = np.argsort(b, kind="stable")
    start = np.zeros(int(b.max()) + 2, np.int64)
    start[1:] = np.cumsum(np.bincount(b, minlength=int(b.max()) + 1))
    pos = np.empty(b.size, np.int64)
    pos[order] = np.arange(b.size) - start[b[order]]
    return torch.from_numpy(pos)


def lstm_weights(rs, H):
    k = 1.0 / math.sqrt(H)
    u = lambda *s: torch.from_numpy(rs.uniform(-k, k, s).astype(np.float32))                         # noqa: E731
    return u(4 * H, 2 * H), u(4 * H, H), u(4 * H), u(4 * H)


@functools.lru_cache(maxsize=2)
def loop_inputs(name):
    """CPU float32 tensors of a loop case.  Strided cases: `xfull` is N x (H + PAD), NaN outside columns 1 .. H, and x is
    that column block (ldx = H + PAD, base one float past a 16-byte boundary)."""
    c = LOOP_BY_NAME[name]
    rs = np.random.RandomState(c.seed)
    v = Bag()
    v.case, v.nb = c, len(c.sizes)
    v.batch = batch_vector(c.sizes, c.sorted_batch, rs)
    n = v.batch.numel()
    x = torch.from_numpy((rs.standard_normal((n, c.H)) * c.xscale).astype(np.float32))
    v.w_ih, v.w_hh, v.b_ih, v.b_hh = lstm_weights(rs, c.H)
    if not c.bias:
        v.b_ih = v.b_hh = None
    v.gout = torch.from_numpy(rs.standard_normal((v.nb, 2 * c.H)).astype(np.float32))
    v.xfull = None
    if c.strided:
        v.xfull = torch.full((n, c.H + PAD), float("nan"))
        v.xfull[:, 1:1 + c.H] = x
        x = v.xfull[:, 1:1 + c.H]
    v.x = x
    return v


def module_inputs(channels):
    """Set2Set(channels, 3) on the graphs of MODULE_SIZES: x, the sorted batch vector, the nn.LSTM's parameters, the
    cotangent on q*."""
    rs = np.random.RandomState(channels)
    v = Bag()
    v.nb = len(MODULE_SIZES)
    v.batch = batch_vector(MODULE_SIZES, True, rs)
    v.x = torch.from_numpy(rs.standard_normal((v.batch.numel(), channels)).astype(np.float32))
    v.w_ih, v.w_hh, v.b_ih, v.b_hh = lstm_weights(rs, channels)
    v.gout = torch.from_numpy(rs.standard_normal((v.nb, 2 * channels)).astype(np.float32))
    return v


def module_reference(channels, dtype=torch.float64):
    v = module_inputs(channels)
    return set2set_restated(v.x, v.batch, v.nb, v.w_ih, v.w_hh, v.b_ih, v.b_hh, 3, v.gout, dtype)


def rows_as_read(v, unstaged_stride=None):
    """The N x H node rows as a kernel reads them out of the flat buffer of a strided case: row i starts at 1 + i * ldx.
    unstaged_stride (alteration c): the rows of the un-staged graphs start at 1 + i * unstaged_stride instead."""
    c = v.case
    n, ldx = v.batch.numel(), c.H + PAD
    flat = v.xfull.reshape(-1)
    stride = torch.full((n,), ldx, dtype=torch.int64)
    if unstaged_stride is not None:
        big = torch.tensor([s * c.H > XCAP for s in c.sizes])
        stride[big[v.batch]] = unstaged_stride
    idx = 1 + torch.arange(n) * stride
    return flat[idx[:, None] + torch.arange(c.H)[None, :]]


# ---- the restatement -----------------------------------------------------------------------------------------------------
FAULTS = ("gate_rows_past_1024_at_bias", "weights_past_1024_unnormalised", "unstaged_rows_stride_h", "no_max_subtraction",
          "dw_hh_from_wrong_columns")


def segment_softmax(e, batch, nb, subtract_max=True, raw_from=None, pos=None):
    """Per-graph softmax of e with max-subtraction.  raw_from (alteration b): nodes at position >= raw_from inside their
    graph keep the un-normalised weight exp(e - m)."""
    if subtract_max:
        with torch.no_grad():
            m = torch.full((nb,), -math.inf, dtype=e.dtype).scatter_reduce(0, batch, e, "amax", include_self=True)
        w = torch.exp(e - m[batch])
    else:
        w = torch.exp(e)
    s = torch.zeros(nb, dtype=e.dtype).index_add(0, batch, w)
    a = w / s[batch]
    if raw_from is not None:
        a = torch.where(pos >= raw_from, w, a)
    return a


def set2set_restated(x, batch, nb, w_ih, w_hh, b_ih, b_hh, T, gout, dtype=torch.float64, fault=None):
    """QC/set2set.py:50-75 in plain torch ops under autograd, in `dtype` on the CPU: for every step the LSTM cell written out
    (gates = W_ih q* + b_ih + W_hh h + b_hh, order i, f, g, o; c' = f c + i g; h' = o tanh c'), e_i = <x_i, q[batch_i]>, the
    per-graph softmax with max-subtraction, r = scatter_add(a x), q* = [q | r].  Returns qs[T + 1], cs[T + 1] (index 0: the
    zero initial state), gates[T] (the four activations), att[T], the logits, and the gradients of x, w_ih, w_hh, b_ih, b_hh
    under the cotangent gout on the final q*.  fault: one of FAULTS, the same arithmetic wrong in one way the kernels could
    be wrong (test_set2set_routes.py holds them against the true one under the GPU test's comparison)."""
    assert fault is None or fault in FAULTS
    H = x.shape[1]
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)       # noqa: E731
    X, Wi, Wh, Bi, Bh = (leaf(t) for t in (x, w_ih, w_hh, b_ih, b_hh))
    pos = position_in_graph(batch) if fault == "weights_past_1024_unnormalised" else None
    q_star = torch.zeros(nb, 2 * H, dtype=dtype)
    h, c = torch.zeros(nb, H, dtype=dtype), torch.zeros(nb, H, dtype=dtype)
    qs, cs, gates, att, logits = [q_star], [c], [], [], []
    for _ in range(T):
        bias = (Bi + Bh) if Bi is not None else torch.zeros(4 * H, dtype=dtype)
        pre = q_star @ Wi.t() + h @ Wh.t() + bias
        if fault == "gate_rows_past_1024_at_bias":
            pre = torch.where(torch.arange(4 * H) >= NT, bias.expand_as(pre), pre)
        i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        e = (X * h[batch]).sum(-1)
        a = segment_softmax(e, batch, nb, subtract_max=fault != "no_max_subtraction",
                            raw_from=NT if fault == "weights_past_1024_unnormalised" else None, pos=pos)
        r = torch.zeros(nb, H, dtype=dtype).index_add(0, batch, a[:, None] * X)
        q_star = torch.cat([h, r], -1)
        qs.append(q_star); cs.append(c); gates.append(torch.cat([i, f, g, o], -1)); att.append(a); logits.append(e)
    (q_star * gout.to(dtype)).sum().backward()
    res = {"qs": torch.stack(qs).detach(), "cs": torch.stack(cs).detach(), "gates": torch.stack(gates).detach(),
           "att": torch.stack(att).detach(), "logits": torch.stack(logits).detach(),
           "dx": X.grad, "dw_ih": Wi.grad, "dw_hh": Wh.grad, "db_ih": None if Bi is None else Bi.grad,
           "db_hh": None if Bh is None else Bh.grad}
    if fault == "dw_hh_from_wrong_columns":
        res["dw_hh"] = Wi.grad[:, H:].clone()
    return res


def loop_reference(name, dtype=torch.float64, fault=None):
    v = loop_inputs(name)
    x = v.x
    if fault == "unstaged_rows_stride_h":
        assert v.case.strided
        x = rows_as_read(v, unstaged_stride=v.case.H)
    return set2set_restated(x, v.batch, v.nb, v.w_ih, v.w_hh, v.b_ih, v.b_hh, v.case.T, v.gout, dtype, fault)


@functools.lru_cache(maxsize=2)
def loop_reference64(name):
    return loop_reference(name)


def segment_attention_restated(x, q, batch, nb, dr, dtype=torch.float64):
    """One processing step's readout (QC/set2set.py:63-74): a = per-graph softmax(<x_i, q_b>), r_b = sum_i a_i x_i, and the
    gradients of x and q under the cotangent dr."""
    X, Q = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, q))
    e = (X * Q[batch]).sum(-1)
    a = segment_softmax(e, batch, nb)
    r = torch.zeros(nb, x.shape[1], dtype=dtype).index_add(0, batch, a[:, None] * X)
    (r * dr.to(dtype)).sum().backward()
    return {"a": a.detach(), "r": r.detach(), "dx": X.grad, "dq": Q.grad, "logits": e.detach()}


@functools.lru_cache(maxsize=2)
def seg_inputs(name):
    c = SEG_BY_NAME[name]
    rs = np.random.RandomState(c.seed)
    v = Bag()
    v.case, v.nb = c, len(c.sizes)
    v.batch = batch_vector(c.sizes, c.sorted_batch, rs)
    n = v.batch.numel()
    x = torch.from_numpy(rs.standard_normal((n, c.h)).astype(np.float32))
    v.q = torch.from_numpy((rs.standard_normal((v.nb, c.h)) * (2.0 / math.sqrt(c.h)) * c.qscale).astype(np.float32))
    v.dr = torch.from_numpy(rs.standard_normal((v.nb, c.h)).astype(np.float32))
    v.xfull = None
    if c.strided:
        v.xfull = torch.full((n, c.h + PAD), float("nan"))
        v.xfull[:, 1:1 + c.h] = x
        x = v.xfull[:, 1:1 + c.h]
    v.x = x
    return v


def seg_reference(name, dtype=torch.float64):
    v = seg_inputs(name)
    return segment_attention_restated(v.x, v.q, v.batch, v.nb, v.dr, dtype)


# ---- the comparison ------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """The metric of the suite's `close`: max |got - ref| / max(1, max |ref|); infinite when anything is not finite or
    the shapes differ."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    if got.shape != ref.shape:
        return math.inf
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs().max().item()
    if not math.isfinite(err):
        return math.inf
    return err / max(1.0, ref.abs().max().item())


def stepwise_err(got, ref):
    """Arrays with a leading step axis: every step against its own scale, the worst of them."""
    if got.shape != ref.shape:
        return math.inf
    return max([rel_err(got[t], ref[t]) for t in range(ref.shape[0])] or [0.0])


def loop_errors(got, ref):
    """{quantity: error} of a loop result (dict with FWD_KEYS and GRAD_KEYS) against the reference."""
    out = {k: stepwise_err(got[k], ref[k]) for k in FWD_KEYS}
    for k in GRAD_KEYS:
        if ref[k] is None:
            assert got[k] is None, k
        else:
            out[k] = rel_err(got[k], ref[k])
    return out


def seg_errors(got, ref):
    return {k: rel_err(got[k], ref[k]) for k in ("a", "r", "dx", "dq")}


def base_tolerances(keys_fwd, keys_grad):
    t = {k: TOL_FWD for k in keys_fwd}
    t.update({k: TOL_GRAD for k in keys_grad})
    return t


def tolerances(base, e32=None):
    """Ordinary cases: the base tolerances.  Large-logit cases: max(base, 4 x e32) per quantity, e32 the float32
    restatement's own error, capped at TOL_CAP (test_set2set_routes.py asserts 4 x e32 <= TOL_CAP: the cap passes nothing)."""
    if e32 is None:
        return dict(base)
    return {k: min(max(t, 4.0 * e32[k]), TOL_CAP) for k, t in base.items()}


LOOP_TOL = base_tolerances(FWD_KEYS, GRAD_KEYS)
SEG_TOL = base_tolerances(("a", "r"), ("dx", "dq"))


def failures(errors, tol):
    """The quantities whose error is above their tolerance (or not a number)."""
    return sorted(k for k, e in errors.items() if not e <= tol[k])


def lstm_tolerances(B, I, H):
    """(forward, backward) for the LSTM cell: the existing 2e-6 and 4e-6 sqrt(B), times max(1, sqrt((I + H) / 400)) - the
    widest contraction held at those numbers is 300 + 100, and a sequential fp32 sum's rounding grows like the square root
    of its length."""
    m = max(1.0, math.sqrt((I + H) / 400.0))
    return LSTM_TOL_FWD * m, LSTM_TOL_GRAD * max(1.0, math.sqrt(B)) * m
