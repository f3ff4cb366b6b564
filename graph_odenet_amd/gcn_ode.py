"""Fused GCN ODE function: f(t, x) = relu( A @ ([t | GroupNorm(x)] @ W) + b )
(reference: ODEfunc.forward, GCN/models.py:172-179 -> FixedGraphConvolution.forward,
GCN/layers.py:69-75) and its vector-Jacobian products, as two / five HIP kernel launches:

  forward   : gode_gn_time_gemm_f32 (stage combine + GroupNorm + time column + MFMA GEMM)
              gode_spmm_csr_f32     (gather-aggregate + bias + relu)
  adjoint   : + relu-masked cotangent in the SpMM epilogue, gode_spmm_csr_f32 on A^T,
              gode_gn_time_gemm_bwd_f32 (dS W^T + GroupNorm backward), gode_wgrad_f32,
              gode_colsum_f32 (bias), gode_reduce_parts_f32 (block partials).

Stage inputs arrive as (coef, tensor) term lists and are combined inside the kernels.
"""
import ctypes

import torch

from . import _lib, ops
from .graph import as_graph
from .solver import Field, adaptive_code, adaptive_stages, method_code, multistep_nfe, n_stages


def _graph_struct(g, d):
    gs = _lib.Graph()
    gs.rowptr, gs.col = g.rowptr.data_ptr(), g.col.data_ptr()
    gs.val = g.val.data_ptr() if g.val is not None else None
    gs.items, gs.n_items = (g.items.data_ptr() if g.items is not None else None), g.n_items
    gs.long_rows = g.long_rows.data_ptr() if g.long_rows is not None else None
    gs.n_long = g.n_long
    part = g.partial(d)
    gs.partial = part.data_ptr() if part is not None else None
    gs.n_rows, gs.nnz = g.n_rows, g.nnz
    return gs


class _Shared:
    """Per-(graph, d) workspaces shared by the forward and adjoint fields."""

    def __init__(self, graph, d, device):
        n = graph.n_rows
        self.S = torch.empty(n, d, dtype=torch.float32, device=device)
        self.dZ = None
        self.dS = None
        self.n = n
        self.d = d
        self.device = device
        self._ky = self._ka = self._kt = None
        self._parts = None
        # rows of the per-block column sums the forward-recompute SpMM of an adjoint stage can leave (0: not on this shape)
        self.y2_rows = 0                       # (a row-partitioned graph runs the per-stage Python path: no per-block sums)
        if not getattr(graph, "is_partitioned", False) and hasattr(graph, "n_items"):
            self.y2_rows = _lib.load().gode_spmm_y2_colsum_rows(graph.n_items if graph.items is not None else n, graph.n_long, d)
        self._y2_colsum = None
        self._X2 = None

    @property
    def X2(self):
        """Pair of n x d arrays the C drivers write combined stage inputs to (csrc/ode_driver.hip)."""
        if self._X2 is None:
            self._X2 = [torch.empty_like(self.S), torch.empty_like(self.S)]
        return self._X2

    def bwd(self):
        if self.dZ is None:
            self.dZ = torch.empty_like(self.S)
            self.dS = torch.empty_like(self.S)
        return self.dZ, self.dS

    # ---- buffers of the C-level rk4 driver (csrc/ode_driver.hip) --------------------------------
    def stage_buffers(self, adjoint):
        if self._ky is None:
            self._ky = [torch.empty_like(self.S) for _ in range(4)]
        if adjoint and self._ka is None:
            lib = _lib.load()
            P = lib.gode_gcn_ode_theta_len(self.d)
            self._ka = [torch.empty_like(self.S) for _ in range(4)]
            self._kt = [torch.empty(P, dtype=torch.float32, device=self.device) for _ in range(4)]
            nW = (self.d + 1) * self.d
            self._parts = (torch.empty(lib.gode_wgrad_parts(self.n) * nW, dtype=torch.float32, device=self.device),
                           torch.empty(lib.gode_gemm_bwd_parts(self.n) * self.d, dtype=torch.float32, device=self.device),
                           torch.empty(lib.gode_gemm_bwd_parts(self.n) * self.d, dtype=torch.float32, device=self.device),
                           torch.empty(max(lib.gode_colsum_scratch_bytes(self.n, self.d), 16), dtype=torch.uint8,
                                       device=self.device))
        return self._ky, self._ka, self._kt, self._parts

    def workspace_struct(self, adjoint, groups=0):
        ky, ka, kt, parts = self.stage_buffers(adjoint)
        ws = _lib.Rk4Workspace()
        ws.S = self.S.data_ptr()
        for i in range(4):
            ws.ky[i] = ky[i].data_ptr()
        if not adjoint and _lib.load().gode_gcn_small_supported(self.n, self.d, int(groups)):
            # launch-bound graphs: the dopri5 step driver chains the stage inputs through this pair (csrc/ode_driver.hip)
            ws.X[0], ws.X[1] = self.X2[0].data_ptr(), self.X2[1].data_ptr()
        if adjoint:
            dZ, dS = self.bwd()
            ws.dZ, ws.dS = dZ.data_ptr(), dS.data_ptr()
            if getattr(self, "S2", None) is None:
                self.S2 = torch.empty_like(self.S)
            ws.S2 = self.S2.data_ptr()
            for i in range(4):
                ws.ka[i] = ka[i].data_ptr()
                ws.ktheta[i] = kt[i].data_ptr()
            ws.wpart, ws.gpart, ws.bpart, ws.colsum_scratch = (p.data_ptr() for p in parts)
            ws.X[0], ws.X[1] = self.X2[0].data_ptr(), self.X2[1].data_ptr()
            sp = self.small_part(groups)
            ws.small_part = sp.data_ptr() if sp is not None else None
            if self.y2_rows > 0:
                if self._y2_colsum is None:
                    self._y2_colsum = torch.empty(self.y2_rows, self.d, dtype=torch.float32, device=self.device)
                ws.y2_colsum = self._y2_colsum.data_ptr()
        return ws

    def adams_extra(self, adjoint):
        """The further n x d arrays the multistep C drivers rotate through (gode_gcn_ode_adams_*): 2 forward, 4 adjoint."""
        n = 4 if adjoint else 2
        have = getattr(self, "_adams_extra", [])
        if len(have) < n:
            self._adams_extra = have = have + [torch.empty_like(self.S) for _ in range(n - len(have))]
        return have[:n]

    def cot_colpart(self):
        """Per-block column sums of the masked cotangent of a backprop sweep (csrc/backprop.hip); None when the width has
        no 16-byte kernel."""
        rows = _lib.load().gode_masked_cot_parts(self.n, self.d)
        if rows <= 0:
            return None
        if getattr(self, "_cot_colpart", None) is None:
            self._cot_colpart = torch.empty(rows, self.d, dtype=torch.float32, device=self.device)
        return self._cot_colpart

    def small_part(self, groups):
        """Block partials of the fused launch-bound VJP (csrc/small.hip); None when the shape is outside that path."""
        lib = _lib.load()
        if not lib.gode_gcn_small_supported(self.n, self.d, int(groups)):
            return None                       # e.g. 2^20 x 128: 277 MB that nothing would ever read
        if getattr(self, "_small_part", None) is None:
            # 7 slots: a dopri5 backprop step that opens an interval closes seven stages at once
            self._small_part = torch.empty(7 * lib.gode_gcn_small_parts(self.n) * lib.gode_gcn_small_part_len(self.d),
                                           dtype=torch.float32, device=self.device)
        return self._small_part


def _func_struct(spec):
    fs = _lib.GcnOdeFunc()
    fs.A = _graph_struct(spec.graph, spec.d)
    fs.AT = _graph_struct(spec.graph.transpose(), spec.d)
    fs.n, fs.d, fs.groups, fs.eps = spec.graph.n_rows, spec.d, spec.groups, spec.eps
    fs.W, fs.b = spec.W.data_ptr(), spec.b.data_ptr()
    fs.gamma, fs.beta = spec.gamma.data_ptr(), spec.beta.data_ptr()
    core = getattr(spec.graph, "_at_core", None)        # A^T's records without the isolated rows (tuned_graph's gate)
    if core is not None:
        fs.at_core_items, fs.at_n_core, fs.at_diag = core.items.data_ptr(), core.n_items, core.diag.data_ptr()
        a = spec.graph.__dict__["_a_core"]
        fs.a_core_items, fs.a_n_core, fs.a_diag = a.items.data_ptr(), a.n_items, a.diag.data_ptr()
        fs.n_tail = spec.graph.__dict__.get("_n_tail", 0)       # rows [n - n_tail, n): all isolated (local_tail_rows)
        head = spec.graph.__dict__.get("_a_head")               # A's records without the tail rows (adjoint_tail)
        if head is not None:
            fs.a_head_items, fs.a_n_head = head.data_ptr(), head.shape[0]
    return fs


E_UNSUPPORTED = -5        # include/graphode.h: GODE_E_UNSUPPORTED


def _by_ptr(ptr_value, candidates):
    for t in candidates:
        if t.data_ptr() == ptr_value:
            return t
    raise RuntimeError("rk4 driver returned an unknown buffer")


# ---- node renumbering of large graphs ("Node order of large graphs") --------------------------
# The aggregation gathers d*4-byte operand rows; which rows are hot is a property of the graph, where they sit in
# memory is ours to choose.  On the R-MAT benchmark graph the hubs are the ids with few one-bits (0, 1, 2, 4, ...): their
# rows share their low address bits, and the same product runs 13-15 % faster with the nodes renumbered hubs first
# (tools/dev/relabel_probe.py; bit-identical state either way: CSRGraph.relabel).
#
# Round 2 decided this with a stopwatch (three timed launches each way, 4 % margin, 1 GB of scratch, a host
# synchronisation) - the same inputs could then integrate on different node orders on different boxes, and parameter
# gradients (sums over the nodes in row order) differ by 2e-5 between the orders.  Since round 3 the decision is a
# function of the graph alone, in integer arithmetic:
#
#   imbalance(order) = max over residues r of  #{gathers whose operand row id = r  (mod m)}  /  (gathers / m),
#                      m = 32 KiB / row bytes (64 at d = 128), over the gathers of A and of A^T
#
# i.e. how unevenly the gathered rows fall on the address bits just above a row.  R-MAT as generated: 10.8; the same
# graph hubs-first: 1.14; a uniform random graph: 1.005.  `node_order`:
#   "auto"   - renumber hubs-first when the operand is past the caches (>= 64 MB, >= 2^21 non-zeros), the given order's
#              imbalance is >= RELABEL_MIN_IMBALANCE and the hubs-first order at least halves it;
#   "given"  - never;   "degree" - always (any size).
# The decision is cached on the graph per (d, node_order) and reported by bench.py.
RELABEL_MIN_OPERAND_BYTES = 64 << 20      # below this the operand sits in the L2s / the Infinity Cache anyway
RELABEL_MIN_NNZ = 1 << 21
RELABEL_MIN_IMBALANCE = 2.0
NODE_ORDERS = ("auto", "given", "degree")


def gather_imbalance(graph, d, inverse=None):
    """The statistic above for `graph` (square CSR) at row width d, optionally under a renumbering (inverse[old] = new).
    Exact integer counts -> the same number on every box.  One device->host copy of 2 m counters."""
    m = max(8, min(4096, (32 << 10) // (4 * d)))
    col = graph.col.to(torch.int64)
    rp = graph.rowptr.to(torch.int64)
    deg = rp[1:] - rp[:-1]                                  # row r is gathered deg(r) times by the product with A^T
    rows = torch.arange(graph.n_rows, device=col.device)
    if inverse is not None:
        col, rows = inverse[col], inverse
    h_a = torch.bincount(col % m, minlength=m)
    h_t = torch.zeros(m, dtype=torch.int64, device=col.device).index_add_(0, rows % m, deg)
    h = torch.stack([h_a, h_t]).tolist()
    return max(max(hh) * m / max(sum(hh), 1) for hh in h)


# ---- diagonal-only rows leave the block's SpMM launches ("Diagonal-only rows") ----------------
# A row whose only entry is its own diagonal costs a product a record, a row read and a row written (16 + 8 + 8 d bytes,
# 1 048 at d = 128) for a scaled copy of a row the launch before it held in registers.  With the core lists
# (CSRGraph.diag_rows / isolated_rows) that launch stores the row itself:
#   adjoint solve   rows isolated in A and A^T leave the product with A^T; the launch that forms dZ stores a_ii dZ[i] into
#                   dS instead of dZ[i] into dZ (same bytes) and loads one dword of the scale per record - a memory sector
#                   of up to 64 bytes each, the rows of neighbouring records not being neighbours;
#   forward solve   rows diagonal-only in A leave the product with A; the dense launch before it stores relu(a_ii S[i] + b)
#                   (512 B more, and 512 B less where the row is isolated and its S row is dropped) and loads two dwords per
#                   row, coalesced.
# At the worst 64 n bytes per adjoint stage and 8 n per forward stage against 1 048 n_isolated saved in each: even at a
# share of 1/16.  The block takes the lists from twice that share on, an exact integer count:
#       8 * n_isolated >= n_rows,    n_rows > 65 536   (csrc/ode_driver.hip uses the lists on the large route only).
# Below that no list is built and nothing changes.  R-MAT 2^20 / 10 M edges with self loops: 45.4 % of the rows.
CORE_LIST_MIN_ROWS = 65536
CORE_LIST_MIN_SHARE_INV = 8


def local_tail_rows(g):
    """n_tail of the ODE block (include/graphode.h: gode_gcn_odefunc_t): the length of the longest suffix of rows of `g` that
    are all isolated - after the hubs-first renumbering of a graph with self loops everywhere that is every isolated row,
    degree sum 2 being the minimum - where it is at least the share of the rows the core lists ask for; else 0.  The forward
    rk4 solve integrates such rows in one row-local launch (csrc/ode_driver.hip, option local_tail)."""
    n_tail = g.isolated_tail()
    return n_tail if CORE_LIST_MIN_SHARE_INV * n_tail >= g.n_rows else 0


def head_items(g, n_tail):
    """A's record list without the records of the rows [n - n_tail, n) (gode_gcn_odefunc_t: a_head_items): the list Sp(g) of
    the adjoint solve walks when the tail rows are recomputed in a dense launch of their own (csrc/ode_driver.hip, option
    adjoint_tail).  None when there is no tail, no more than CORE_LIST_MIN_ROWS rows before it (the driver's large route
    starts above that), or when the tail's records are not the last n_tail of the list in row order (a graph with empty
    rows: their records sort behind the one-entry ones) - the driver wants the head to be a prefix of the list, so that the
    tail launch can leave the per-block column sums the whole list would have.  Exact integer comparisons."""
    if n_tail <= 0 or g.n_rows - n_tail <= CORE_LIST_MIN_ROWS or g.items is None:
        return None
    n_head = g.n_items - n_tail                                       # every tail row is isolated, hence one record
    want = torch.arange(g.n_rows - n_tail, g.n_rows, dtype=g.items.dtype, device=g.items.device)
    if n_head <= 0 or not torch.equal(g.items[n_head:, 0], want):
        return None
    return g.items[:n_head]


def _hand_core_list(g, info):
    """Decide (from counts alone) whether the ODE block gets the core lists of A and A^T; if so build them on `g`."""
    if getattr(g, "items", None) is None or g.n_rows <= CORE_LIST_MIN_ROWS or g.transpose().items is None:
        return
    if "_at_core" not in g.__dict__:
        iso = g.transpose().isolated_rows()
        take = CORE_LIST_MIN_SHARE_INV * iso.n_flagged >= g.n_rows and iso.n_items > 0
        if take:
            iso.items                                               # built here, once, not inside a solve
            g.diag_rows().items
        g.__dict__["_at_core"] = iso if take else None
        g.__dict__["_a_core"] = g.diag_rows() if take else None      # A's list for the forward solve: every diagonal-only row of A
        g.__dict__["_isolated_count"] = iso.n_flagged
        g.__dict__["_n_tail"] = local_tail_rows(g) if take else 0
        g.__dict__["_a_head"] = head_items(g, g.__dict__["_n_tail"])
    head = g.__dict__["_a_head"]
    info.update(isolated_rows=g.__dict__["_isolated_count"], core_lists=g.__dict__["_at_core"] is not None,
                n_tail=g.__dict__["_n_tail"], head_records=0 if head is None else int(head.shape[0]))


def tuned_graph(graph, d, node_order="auto"):
    """(graph the ODE block should integrate on, order, inverse) - order is None when the graph is used as given.
    y' = y[order] are the state rows in the renumbered graph; y = y'[inverse].  Deterministic in (graph, d, node_order)."""
    if node_order not in NODE_ORDERS:
        raise ValueError("node_order must be one of %s, got %r" % (NODE_ORDERS, node_order))
    cache = graph.__dict__.setdefault("_tuned", {})
    hit = cache.get((d, node_order))
    if hit is not None:
        return hit
    res = (graph, None, None)
    info = {"node_order": node_order, "renumbered": False}
    square = graph.n_rows == graph.n_cols and not getattr(graph, "is_partitioned", False)
    big = graph.n_rows * d * 4 >= RELABEL_MIN_OPERAND_BYTES and graph.nnz >= RELABEL_MIN_NNZ
    if square and node_order != "given" and (node_order == "degree" or big) \
            and not torch.cuda.is_current_stream_capturing():
        order = graph.degree_order()
        inverse = torch.empty_like(order)
        inverse[order] = torch.arange(graph.n_rows, device=graph.device)
        take = node_order == "degree"
        if not take:
            given, hubs = gather_imbalance(graph, d), gather_imbalance(graph, d, inverse)
            info.update(imbalance_given=round(given, 4), imbalance_hubs_first=round(hubs, 4))
            take = given >= RELABEL_MIN_IMBALANCE and hubs <= 0.5 * given
        if take:
            res = (graph.relabel(order), order, inverse)
            info["renumbered"] = True
    if square and not (res[0].device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        _hand_core_list(res[0], info)
    graph.__dict__.setdefault("_tuned_info", {})[(d, node_order)] = info
    cache[(d, node_order)] = res
    return res


class GcnOdeSpec:
    """Plain description of one ODEfunc instance (tensors are the live parameters)."""

    def __init__(self, graph, W, b, gamma, beta, groups, eps):
        self.graph, self.W, self.b, self.gamma, self.beta = graph, W, b, gamma, beta
        self.groups, self.eps = int(groups), float(eps)
        self.d = W.shape[1]
        if W.shape[0] != self.d + 1:
            raise ValueError("GcnOdeSpec: weight must be (d+1) x d, got %s" % (tuple(W.shape),))
        if graph.n_rows != graph.n_cols:
            raise ValueError("GcnOdeSpec: adjacency must be square")


def small_fused(spec):
    """True when the launch-bound one-launch f-eval / VJP of csrc/small.hip applies (and is switched on)."""
    lib = _lib.load()
    return bool(lib.gode_get_option(b"small_fused") == 1 and not getattr(spec.graph, "is_partitioned", False)
                and lib.gode_gcn_small_supported(spec.graph.n_rows, spec.d, spec.groups))


def _feval_small(spec, t, terms, out, pre=None, alpha=1.0, cot=None, out2=None, next_terms=None, x_next=None):
    """next_terms / x_next: the launch also writes the next stage's combined input (a term that is `out` itself is this
    launch's result) - what the C dopri5 step driver does between its stages."""
    lib = _lib.load()
    fs = _func_struct(spec)
    lx = _lib.lincomb(terms)
    lp = _lib.lincomb(pre) if pre is not None else None
    lc = _lib.lincomb(cot) if cot is not None else None
    ln = _lib.lincomb(next_terms) if next_terms is not None else None
    _lib.check(lib.gode_gcn_feval_small_next_f32(ctypes.byref(fs), ctypes.byref(lx), float(t), float(alpha),
                                                 ctypes.byref(lp) if lp is not None else None,
                                                 ctypes.byref(lc) if lc is not None else None,
                                                 _lib.ptr(out2) if cot is not None else None, _lib.ptr(out),
                                                 ctypes.byref(ln) if ln is not None else None,
                                                 _lib.ptr(x_next) if ln is not None else None, _lib.stream_ptr()),
               "gode_gcn_feval_small_next_f32")


def _byref(lc):
    return ctypes.byref(lc) if lc is not None else None


def _feval_small_save(spec, t, terms, out, k, pre=None, alpha=1.0):
    """The same evaluation, which also stores relu(z) into k (the launch that closes a step of a backprop solve)."""
    lib = _lib.load()
    fs = _func_struct(spec)
    lx = _lib.lincomb(terms)
    lp = _lib.lincomb(pre) if pre is not None else None
    _lib.check(lib.gode_gcn_feval_small_save_f32(ctypes.byref(fs), ctypes.byref(lx), float(t), float(alpha), _byref(lp),
                                                 _lib.ptr(out), _lib.ptr(k), _lib.stream_ptr()),
               "gode_gcn_feval_small_save_f32")


def _vjp_small(spec, terms, dZ, ka, part, pre=None, out_scale=1.0, fs=None):
    """ka = (sum pre) + out_scale * dx and the block partial rows (gode_gcn_small_parts x gode_gcn_small_part_len) of one
    stage, from the masked cotangent dZ."""
    lib = _lib.load()
    fs = _func_struct(spec) if fs is None else fs
    lx = _lib.lincomb(terms)
    lp = _lib.lincomb(pre) if pre is not None else None
    _lib.check(lib.gode_gcn_vjp_small_f32(ctypes.byref(fs), ctypes.byref(lx), _lib.ptr(dZ), float(out_scale), _byref(lp),
                                          _lib.ptr(ka), _lib.ptr(part), _lib.stream_ptr()), "gode_gcn_vjp_small_f32")


def _vjp_small_next(spec, terms, dZ, ka, part, cot_next, k_next, dZ_next, pre=None, out_scale=1.0):
    """The same launch, which also writes dZ_next = (sum cot_next) * [k_next > 0] (a term of cot_next that is `ka` itself
    is this launch's result) - what the reverse sweep of a backprop solve does between its stages."""
    lib = _lib.load()
    fs = _func_struct(spec)
    lx = _lib.lincomb(terms)
    lp = _lib.lincomb(pre) if pre is not None else None
    ln = _lib.lincomb(cot_next)
    _lib.check(lib.gode_gcn_vjp_small_next_f32(ctypes.byref(fs), ctypes.byref(lx), _lib.ptr(dZ), float(out_scale), _byref(lp),
                                               _lib.ptr(ka), _lib.ptr(part), ctypes.byref(ln), _lib.ptr(k_next),
                                               _lib.ptr(dZ_next), _lib.stream_ptr()), "gode_gcn_vjp_small_next_f32")


def _finish_small(spec, part, ktheta, t, fs=None):
    """ktheta = [W (row 0 scaled by t) | b | gamma | beta | a_t] of one stage from its block partial rows."""
    lib = _lib.load()
    fs = _func_struct(spec) if fs is None else fs
    _lib.check(lib.gode_gcn_small_finish_f32(ctypes.byref(fs), _lib.ptr(part), _lib.ptr(ktheta), float(t),
                                             _lib.stream_ptr()), "gode_gcn_small_finish_f32")


def _finish_small_multi(spec, part, kthetas, ts):
    """len(kthetas) <= 8 stages at once; `part` holds their partial buffers back to back."""
    lib = _lib.load()
    fs = _func_struct(spec)
    n = len(kthetas)
    _lib.check(lib.gode_gcn_small_finish_multi_f32(ctypes.byref(fs), _lib.ptr(part), n,
                                                   (ctypes.c_void_p * n)(*[k.data_ptr() for k in kthetas]),
                                                   (ctypes.c_float * n)(*[float(t) for t in ts]), _lib.stream_ptr()),
               "gode_gcn_small_finish_multi_f32")


def _finish_small4(spec, part, theta, wb, ts):
    """theta += sum_s wb[s] * (stage s of _finish_small at ts[s]) over the four partial buffers held back to back in `part`."""
    lib = _lib.load()
    fs = _func_struct(spec)
    wbh, tsh = (ctypes.c_float * 4)(*[float(v) for v in wb]), (ctypes.c_float * 4)(*[float(v) for v in ts])
    _lib.check(lib.gode_gcn_small_finish4_f32(ctypes.byref(fs), _lib.ptr(part), _lib.ptr(theta), wbh, tsh, _lib.stream_ptr()),
               "gode_gcn_small_finish4_f32")


class _PackedParams:
    """The one statement of the packed parameter buffer the C drivers read and add to: [W | b | gamma | beta | a_t]
    (gode_gcn_ode_theta_len floats).  Needs self.s (the spec) and self.params_order (list of 'gamma', 'beta', 'W', 'b' in
    func.parameters() order)."""

    def _theta_len(self):
        return (self.s.d + 1) * self.s.d + 3 * self.s.d + 1

    def _packed_state(self, th, y, a):
        """[y, a, a_t, W, b, gamma, beta] with the small components as views of the packed buffer th."""
        d = self.s.d
        nW = (d + 1) * d
        comps = [y, a, th[nW + 3 * d:], th[:nW].view(d + 1, d), th[nW:nW + d], th[nW + d:nW + 2 * d],
                 th[nW + 2 * d:nW + 3 * d]]
        comps[2]._gode_packed = th            # keeps the base alive and lets the native step find it
        return comps

    def _in_params_order(self, comps):
        m = {"W": comps[3], "b": comps[4], "gamma": comps[5], "beta": comps[6]}
        return [m[k] for k in self.params_order]

    def packed_grads(self, device):
        """A zeroed packed buffer for the backprop sweeps to add the parameter gradients to."""
        return torch.zeros(self._theta_len(), dtype=torch.float32, device=device)

    def packed_param_grads(self, theta):
        """Views of such a buffer, in func.parameters() order."""
        return self._in_params_order(self._packed_state(theta, None, None))


class GcnOdeField(_PackedParams, Field):
    n_components = 1
    fused = True

    def __init__(self, spec, shared, params_order):
        self.s, self.w = spec, shared
        self.params_order = params_order
        self.token = ("gcn", id(spec.graph))     # identity of the problem besides shapes and parameters (odeint plans)

    def eval(self, t, terms, out):
        s, w = self.s, self.w
        if small_fused(s):
            return _feval_small(s, t, terms[0], out[0])
        ops.gn_time_gemm(terms[0], w.n, s.d, s.groups, s.eps, s.gamma, s.beta, s.W, True, t, out=w.S)
        ops.spmm(s.graph, w.S, bias=s.b, relu=True, out=out[0])

    def rk4_native(self, comps, t0, t1, n_steps):
        """Whole fixed-grid solve in one C call (csrc/ode_driver.hip); comps[0] is re-bound to the result."""
        lib = _lib.load()
        s, w = self.s, self.w
        ky = w.stage_buffers(False)[0]
        fs, ws = _func_struct(s), w.workspace_struct(False, s.groups)
        res = ctypes.c_void_p()
        _lib.check(lib.gode_gcn_ode_rk4_forward(ctypes.byref(fs), _lib.ptr(comps[0]), ctypes.byref(res), ctypes.byref(ws),
                                                float(t0), float(t1), int(n_steps), _lib.stream_ptr()),
                   "gode_gcn_ode_rk4_forward")
        out = _by_ptr(res.value, [comps[0]] + ky)
        if out is not comps[0]:
            # keep the driver's buffers private to the workspace: hand back a copy in the caller's tensor
            comps[0].copy_(out)
        return 4 * n_steps

    def fixed_native(self, comps, t0, t1, n_steps, method):
        """rk4_native for any fixed-grid method (gode_gcn_ode_fixed_forward)."""
        lib = _lib.load()
        s, w = self.s, self.w
        ky = w.stage_buffers(False)[0]
        fs, ws = _func_struct(s), w.workspace_struct(False, s.groups)
        res = ctypes.c_void_p()
        _lib.check(lib.gode_gcn_ode_fixed_forward(method_code(method), ctypes.byref(fs), _lib.ptr(comps[0]), ctypes.byref(res),
                                                  ctypes.byref(ws), float(t0), float(t1), int(n_steps), _lib.stream_ptr()),
                   "gode_gcn_ode_fixed_forward")
        out = _by_ptr(res.value, [comps[0]] + ky)
        if out is not comps[0]:
            comps[0].copy_(out)
        return n_stages(method) * n_steps

    def multistep_native(self, comps, t0, t1, n_steps, method):
        """The whole solve of a multistep method in one C call (gode_gcn_ode_adams_forward), every route."""
        lib = _lib.load()
        s, w = self.s, self.w
        ky, extra = w.stage_buffers(False)[0], w.adams_extra(False)
        fs, ws = _func_struct(s), w.workspace_struct(False, s.groups)
        res = ctypes.c_void_p()
        _lib.check(lib.gode_gcn_ode_adams_forward(ctypes.byref(fs), _lib.ptr(comps[0]), ctypes.byref(res), ctypes.byref(ws),
                                                  (ctypes.c_void_p * 2)(*[x.data_ptr() for x in extra]), float(t0), float(t1),
                                                  int(n_steps), _lib.stream_ptr()), "gode_gcn_ode_adams_forward")
        out = _by_ptr(res.value, [comps[0]] + ky + extra)
        if out is not comps[0]:
            comps[0].copy_(out)
        return multistep_nfe(method, n_steps)

    @staticmethod
    def multistep_record_floats(method, n_steps, step, nd):
        """Floats in front of step's record in the compact record of a multistep solve (step = n_steps: the total): a start-up
        step keeps [y | k_1..k_4], a later step [y | f]."""
        return int(_lib.load().gode_adams_record_offset(int(step), int(nd)))

    def multistep_forward_save(self, method, y0, y_end, save, t0, t1, n_steps, i0, i1, hist=None):
        """Steps i0 .. i1-1 of the solve into the flat record `save` (which starts at step i0's record), multistep_native's
        launches on other addresses; hist: f of the steps i0-1, i0-2, i0-3 where a multistep step needs them."""
        lib = _lib.load()
        s, w = self.s, self.w
        fs, ws = _func_struct(s), w.workspace_struct(False, s.groups)
        hp = None if hist is None else (ctypes.c_void_p * 3)(*[None if x is None else x.data_ptr() for x in (list(hist) + [None] * 3)[:3]])
        _lib.check(lib.gode_gcn_ode_adams_forward_save(ctypes.byref(fs), _lib.ptr(y0), _lib.ptr(y_end), _lib.ptr(save), hp,
                                                       ctypes.byref(ws), float(t0), float(t1), int(n_steps), int(i0), int(i1),
                                                       _lib.stream_ptr()), "gode_gcn_ode_adams_forward_save")

    def multistep_backprop(self, method, save, a, theta, t0, t1, n_steps, rerun=None):
        """The reverse sweep over a whole interval's records (gode_gcn_ode_adams_backprop); rerun: a one-step rk4 record to
        re-run the start-up steps into, `save` then holding their y_i alone.  Returns the tensor holding dL/dy_0 (`a` or one
        of the work arrays)."""
        lib = _lib.load()
        s, w = self.s, self.w
        ka = w.stage_buffers(True)[1]
        work = w.adams_extra(True)
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        res = ctypes.c_void_p()
        _lib.check(lib.gode_gcn_ode_adams_backprop(ctypes.byref(fs), _lib.ptr(save), _lib.ptr(rerun), _lib.ptr(a), _lib.ptr(theta),
                                                   ctypes.byref(res), ctypes.byref(ws), _lib.ptr(w.cot_colpart()),
                                                   (ctypes.c_void_p * 4)(*[x.data_ptr() for x in work]), float(t0), float(t1),
                                                   int(n_steps), _lib.stream_ptr()), "gode_gcn_ode_adams_backprop")
        return _by_ptr(res.value, [a] + work + ka)

    # ---- backprop through a fixed-grid solve (odeint._OdeintBackprop; csrc/ode_driver.hip) ---------------------
    def fixed_forward_save(self, method, y0, y_end, save, t0, t1, n_steps, i0, i1):
        """Steps i0 .. i1-1 of the n_steps-step solve from t0 to t1, bit for bit fixed_native's launches (rk4: rk4_native's);
        save[r] = [y_n, k_1..k_S] of step i0 + r (y0 is copied into save[0][0] unless it is that slice)."""
        lib = _lib.load()
        s, w = self.s, self.w
        fs, ws = _func_struct(s), w.workspace_struct(False, s.groups)
        _lib.check(lib.gode_gcn_ode_fixed_forward_save(method_code(method), ctypes.byref(fs), _lib.ptr(y0), _lib.ptr(y_end),
                                                       _lib.ptr(save), ctypes.byref(ws), float(t0), float(t1), int(n_steps),
                                                       int(i0), int(i1), _lib.stream_ptr()), "gode_gcn_ode_fixed_forward_save")

    def fixed_backprop(self, method, save, a, theta, t0, t1, n_steps, i0, i1):
        """Reverse sweep over the records of fixed_forward_save: `a` (dL/dy after step i1-1) is overwritten; returns the
        tensor holding dL/dy before step i0 (`a` or a workspace buffer); theta (packed [W | b | gamma | beta | .]) is
        incremented by the parameter gradients."""
        lib = _lib.load()
        s, w = self.s, self.w
        ka = w.stage_buffers(True)[1]
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        res = ctypes.c_void_p()
        _lib.check(lib.gode_gcn_ode_fixed_backprop(method_code(method), ctypes.byref(fs), _lib.ptr(save), _lib.ptr(a),
                                                   _lib.ptr(theta), ctypes.byref(res), ctypes.byref(ws),
                                                   _lib.ptr(w.cot_colpart()), float(t0), float(t1), int(n_steps), int(i0),
                                                   int(i1), _lib.stream_ptr()), "gode_gcn_ode_fixed_backprop")
        return _by_ptr(res.value, [a] + ka)

    def rk4_forward_save(self, y0, y_end, save, t0, t1, n_steps, i0, i1):
        self.fixed_forward_save("rk4", y0, y_end, save, t0, t1, n_steps, i0, i1)

    def rk4_backprop(self, save, a, theta, t0, t1, n_steps, i0, i1):
        return self.fixed_backprop("rk4", save, a, theta, t0, t1, n_steps, i0, i1)

    def eval_combine(self, t, terms, pre, coef, out):
        """Last RK stage: out[0] = (sum pre[0]) + coef * f(t, sum terms[0]) without materialising f."""
        s, w = self.s, self.w
        if small_fused(s):
            _feval_small(s, t, terms[0], out[0], pre=pre[0], alpha=coef)
            return (0,)
        ops.gn_time_gemm(terms[0], w.n, s.d, s.groups, s.eps, s.gamma, s.beta, s.W, True, t, out=w.S)
        ops.spmm(s.graph, w.S, bias=s.b, relu=True, out=out[0], pre_terms=pre[0], alpha=coef)
        return (0,)

    def dopri5_step_native(self, y, kk, y1, t, h, rtol, atol):
        """One adaptive step in one C call (csrc/ode_driver.hip); returns the error sums as an fp64 device tensor."""
        lib = _lib.load()
        s, w = self.s, self.w
        fs, ws = _func_struct(s), w.workspace_struct(False, s.groups)
        kptr = (ctypes.c_void_p * 7)(*[kk[i][0].data_ptr() for i in range(7)])
        sums = torch.empty(1, dtype=torch.float64, device=y[0].device)
        sc = ops._scratch(y[0].device, lib.gode_rk_errnorm_scratch_bytes())
        _lib.check(lib.gode_gcn_ode_dopri5_step_forward(ctypes.byref(fs), _lib.ptr(y[0]), kptr, _lib.ptr(y1[0]),
                                                        ctypes.byref(ws), float(t), float(h), float(rtol), float(atol),
                                                        _lib.ptr(sums), _lib.ptr(sc), _lib.stream_ptr()),
                   "gode_gcn_ode_dopri5_step_forward")
        return sums

    def adaptive_step_native(self, method, y, kk, y1, t, h, rtol, atol):
        """dopri5_step_native for any adaptive method (kk: S stage buffers): gode_gcn_ode_adaptive_step_forward, which closes
        the step with the fused launch (solution and error sum from one pass over the stages)."""
        lib = _lib.load()
        s, w = self.s, self.w
        S = adaptive_stages(method)
        fs, ws = _func_struct(s), w.workspace_struct(False, s.groups)
        kptr = (ctypes.c_void_p * S)(*[kk[i][0].data_ptr() for i in range(S)])
        sums = torch.empty(1, dtype=torch.float64, device=y[0].device)
        sc = ops._scratch(y[0].device, lib.gode_rk_close_err_scratch_bytes())
        _lib.check(lib.gode_gcn_ode_adaptive_step_forward(adaptive_code(method), ctypes.byref(fs), _lib.ptr(y[0]), kptr,
                                                          _lib.ptr(y1[0]), ctypes.byref(ws), float(t), float(h), float(rtol),
                                                          float(atol), _lib.ptr(sums), _lib.ptr(sc), _lib.stream_ptr()),
                   "gode_gcn_ode_adaptive_step_forward")
        return sums

    # ---- backprop through an adaptive solve (odeint._OdeintBackpropDopri5; csrc/ode_driver.hip) ------------------
    def dopri5_backprop_work(self, like):
        return self.adaptive_backprop_work("dopri5", like)

    def dopri5_step_backprop(self, y, k, g, kbar7, wy, wk, t, h, first, work, turn, theta):
        return self.adaptive_step_backprop("dopri5", y, k, g, kbar7, wy, wk, t, h, first, work, turn, theta)

    def adaptive_backprop_work(self, method, like):
        """Work arrays of adaptive_step_backprop for a state like `like`: S Ybar, two (ybar_n, kbar_1) pairs that take
        turns from step to step, S packed parameter parts."""
        lib = _lib.load()
        S = adaptive_stages(method)
        P = lib.gode_gcn_ode_theta_len(self.s.d)
        return {"ybar": [torch.empty_like(like) for _ in range(S)],
                "pairs": [(torch.empty_like(like), torch.empty_like(like)) for _ in range(2)],
                "ktheta": [torch.empty(P, dtype=torch.float32, device=like.device) for _ in range(S)]}

    def adaptive_step_backprop(self, method, y, k, g, kbar_last, wy, wk, t, h, first, work, turn, theta):
        """Reverse sweep over one accepted step (y_n, k_1..k_S, t_n, h) with cotangent g, weights wy / wk[S] and the
        cotangent kbar_last arriving on k_S (None: none); theta (packed [W | b | gamma | beta | .]) is incremented.
        Returns (ybar_n, kbar_1) in work["pairs"][turn]; kbar_1 is None when `first` (it went through f here).
        gode_gcn_ode_adaptive_step_backprop."""
        lib = _lib.load()
        s, w = self.s, self.w
        S = adaptive_stages(method)
        w.stage_buffers(True)
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        arr = lambda ts: (ctypes.c_void_p * S)(*[x.data_ptr() for x in ts])      # noqa: E731
        ybar_n, kbar1 = work["pairs"][turn]
        _lib.check(lib.gode_gcn_ode_adaptive_step_backprop(
            adaptive_code(method), ctypes.byref(fs), _lib.ptr(y), arr(k), _lib.ptr(g), _lib.ptr(kbar_last), float(wy),
            (ctypes.c_double * S)(*[float(v) for v in wk]), float(t), float(h), int(bool(first)), arr(work["ybar"]),
            _lib.ptr(ybar_n), _lib.ptr(kbar1), _lib.ptr(theta), arr(work["ktheta"]), ctypes.byref(ws),
            _lib.ptr(w.cot_colpart()), _lib.stream_ptr()), "gode_gcn_ode_adaptive_step_backprop")
        return ybar_n, (None if first else kbar1)


class _PartMixin:
    """Row-partitioned state (partition.py): hooks the adaptive solver uses to see global error norms."""
    rk4_native = None
    fixed_native = None
    multistep_native = None
    dopri5_step_native = None
    adaptive_step_native = None
    adaptive = False                # set by odeint when the method is adaptive

    def _part(self):
        return self.s.graph.part

    def global_numel(self, c, t):
        # the big components are row slices (padding rows of a ragged partition count: they are integrated too)
        return t.numel() * self._part().world if c in self.big_components else t.numel()

    def reduce_error_sums(self, sums):
        """Per-component sums of squares -> sums over the ranks for the row-sliced components; the small components
        are already global in adaptive mode."""
        from .partition import global_sum
        p = self._part()
        if p.world == 1:
            return sums
        big = self.big_components
        t = torch.tensor([sums[c] for c in big], dtype=torch.float64, device=self.w.S.device)
        t = global_sum(t, p.group).tolist()
        out = list(sums)
        for c, v in zip(big, t):
            out[c] = v
        return out

    def reduce_small(self, t):
        from .partition import global_sum
        return global_sum(t, self._part().group)


class GcnOdePartField(_PartMixin, GcnOdeField):
    """The same field on a row-partitioned graph (partition.py): ops.spmm gathers the operand rows between the two
    launches of an f-eval, so the whole-solve C drivers are not offered and the solver takes the per-stage path."""
    big_components = (0,)
    rk4_forward_save = None
    rk4_backprop = None
    fixed_forward_save = None
    fixed_backprop = None
    multistep_forward_save = None
    multistep_backprop = None
    dopri5_step_backprop = None
    adaptive_step_backprop = None

    def __init__(self, spec, shared, params_order):
        GcnOdeField.__init__(self, spec, shared, params_order)
        self.token = None


class GcnOdeAdjointField(_PackedParams, Field):
    """Components: [y, a, a_t, W, b, gamma, beta] (b may be absent -> never, FixedGC always has bias here)."""
    fused = True

    def __init__(self, spec, shared, params_order):
        self.s, self.w = spec, shared
        self.params_order = params_order
        self.n_components = 7
        self.ratio_groups = [[0], [1], [2], [3, 4, 5, 6]]

    def new_state(self, y_end):
        """[y, a, a_t, W, b, gamma, beta]; the small components are views of ONE packed buffer laid out as the
        C driver expects: [W | b | gamma | beta | a_t]."""
        self.theta = self.packed_grads(y_end.device)
        return self._packed_state(self.theta, y_end.clone(), torch.zeros_like(y_end))

    def rk4_native(self, comps, t0, t1, n_steps):
        lib = _lib.load()
        s, w = self.s, self.w
        ky, ka, _, _ = w.stage_buffers(True)
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        yr, ar = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.gode_gcn_ode_rk4_adjoint(ctypes.byref(fs), _lib.ptr(comps[0]), _lib.ptr(comps[1]), _lib.ptr(self.theta),
                                                ctypes.byref(yr), ctypes.byref(ar), ctypes.byref(ws),
                                                float(t0), float(t1), int(n_steps), _lib.stream_ptr()),
                   "gode_gcn_ode_rk4_adjoint")
        yo = _by_ptr(yr.value, [comps[0]] + ky)
        ao = _by_ptr(ar.value, [comps[1]] + ka)
        if yo is not comps[0]:
            comps[0].copy_(yo)
        if ao is not comps[1]:
            comps[1].copy_(ao)
        return 4 * n_steps

    def fixed_native(self, comps, t0, t1, n_steps, method):
        """The whole adjoint solve of any fixed-grid method on the launch-bound route (gode_gcn_ode_fixed_adjoint); None
        off that route: the per-stage driver then runs it (the two-chain schedule of large graphs is rk4's alone)."""
        if method == "rk4":
            return self.rk4_native(comps, t0, t1, n_steps)
        lib = _lib.load()
        s, w = self.s, self.w
        ky, ka, _, _ = w.stage_buffers(True)
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        yr, ar = ctypes.c_void_p(), ctypes.c_void_p()
        rc = lib.gode_gcn_ode_fixed_adjoint(method_code(method), ctypes.byref(fs), _lib.ptr(comps[0]), _lib.ptr(comps[1]),
                                            _lib.ptr(self.theta), ctypes.byref(yr), ctypes.byref(ar), ctypes.byref(ws),
                                            float(t0), float(t1), int(n_steps), _lib.stream_ptr())
        if rc == E_UNSUPPORTED:
            return None
        _lib.check(rc, "gode_gcn_ode_fixed_adjoint")
        yo = _by_ptr(yr.value, [comps[0]] + ky)
        ao = _by_ptr(ar.value, [comps[1]] + ka)
        if yo is not comps[0]:
            comps[0].copy_(yo)
        if ao is not comps[1]:
            comps[1].copy_(ao)
        return n_stages(method) * n_steps

    def multistep_native(self, comps, t0, t1, n_steps, method):
        """The whole adjoint solve of a multistep method on the launch-bound route (gode_gcn_ode_adams_adjoint); None off
        that route: solver.integrate_multistep then runs the steps."""
        lib = _lib.load()
        s, w = self.s, self.w
        ky, ka, _, _ = w.stage_buffers(True)
        extra = w.adams_extra(True)
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        yr, ar = ctypes.c_void_p(), ctypes.c_void_p()
        rc = lib.gode_gcn_ode_adams_adjoint(ctypes.byref(fs), _lib.ptr(comps[0]), _lib.ptr(comps[1]), _lib.ptr(self.theta),
                                            ctypes.byref(yr), ctypes.byref(ar), ctypes.byref(ws),
                                            (ctypes.c_void_p * 4)(*[x.data_ptr() for x in extra]), float(t0), float(t1),
                                            int(n_steps), _lib.stream_ptr())
        if rc == E_UNSUPPORTED:
            return None
        _lib.check(rc, "gode_gcn_ode_adams_adjoint")
        yo = _by_ptr(yr.value, [comps[0]] + ky + extra[:2])
        ao = _by_ptr(ar.value, [comps[1]] + ka + extra[2:])
        if yo is not comps[0]:
            comps[0].copy_(yo)
        if ao is not comps[1]:
            comps[1].copy_(ao)
        return multistep_nfe(method, n_steps)

    def param_grads(self, comps):
        return self._in_params_order(comps)

    def _packed_like(self, y):
        """A work copy of the state with the small components as views of ONE packed buffer, as new_state lays it out."""
        th = torch.empty(self._theta_len(), dtype=torch.float32, device=y[0].device)
        return self._packed_state(th, torch.empty_like(y[0]), torch.empty_like(y[1]))

    def alloc_like(self, y, n):
        return [self._packed_like(y) for _ in range(n)]

    @staticmethod
    def _theta_of(comps):
        th = getattr(comps[2], "_gode_packed", None)
        if th is None:
            raise RuntimeError("adjoint state is not in the packed layout")
        return th

    def dopri5_step_native(self, y, kk, y1, t, h, rtol, atol):
        lib = _lib.load()
        s, w = self.s, self.w
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        arr = lambda idx: (ctypes.c_void_p * 7)(*[kk[i][idx].data_ptr() for i in range(7)])      # noqa: E731
        kth = (ctypes.c_void_p * 7)(*[self._theta_of(kk[i]).data_ptr() for i in range(7)])
        sums = torch.empty(4, dtype=torch.float64, device=y[0].device)
        sc = ops._scratch(y[0].device, lib.gode_rk_errnorm_scratch_bytes())
        _lib.check(lib.gode_gcn_ode_dopri5_step_adjoint(
            ctypes.byref(fs), _lib.ptr(y[0]), _lib.ptr(y[1]), _lib.ptr(self._theta_of(y)), arr(0), arr(1), kth,
            _lib.ptr(y1[0]), _lib.ptr(y1[1]), _lib.ptr(self._theta_of(y1)), ctypes.byref(ws), float(t), float(h),
            float(rtol), float(atol), _lib.ptr(sums), _lib.ptr(sc), _lib.stream_ptr()), "gode_gcn_ode_dopri5_step_adjoint")
        return sums

    def adaptive_step_native(self, method, y, kk, y1, t, h, rtol, atol):
        """dopri5_step_native for any adaptive method: gode_gcn_ode_adaptive_step_adjoint, whose one fused close writes the
        three outputs and forms the four error sums."""
        lib = _lib.load()
        s, w = self.s, self.w
        S = adaptive_stages(method)
        fs, ws = _func_struct(s), w.workspace_struct(True, s.groups)
        arr = lambda idx: (ctypes.c_void_p * S)(*[kk[i][idx].data_ptr() for i in range(S)])      # noqa: E731
        kth = (ctypes.c_void_p * S)(*[self._theta_of(kk[i]).data_ptr() for i in range(S)])
        sums = torch.empty(4, dtype=torch.float64, device=y[0].device)
        sc = ops._scratch(y[0].device, lib.gode_rk_close_err_scratch_bytes())
        _lib.check(lib.gode_gcn_ode_adaptive_step_adjoint(
            adaptive_code(method), ctypes.byref(fs), _lib.ptr(y[0]), _lib.ptr(y[1]), _lib.ptr(self._theta_of(y)), arr(0), arr(1),
            kth, _lib.ptr(y1[0]), _lib.ptr(y1[1]), _lib.ptr(self._theta_of(y1)), ctypes.byref(ws), float(t), float(h),
            float(rtol), float(atol), _lib.ptr(sums), _lib.ptr(sc), _lib.stream_ptr()), "gode_gcn_ode_adaptive_step_adjoint")
        return sums

    def eval(self, t, terms, out):
        self._stage(t, terms, out, None, 0.0)

    def eval_combine(self, t, terms, pre, coef, out):
        """Last RK stage: the new y and a are written by the producing launches (SpMM epilogue / GEMM-VJP
        epilogue); the small components get their k in `out` and are combined by the caller."""
        self._stage(t, terms, out, pre, coef)
        return (0, 1)

    def _stage(self, t, terms, out, pre, coef):
        s, w = self.s, self.w
        dZ, dS = w.bwd()
        n, d = w.n, s.d
        y_terms = terms[0]
        packed = getattr(out[2], "_gode_packed", None)
        if packed is not None and small_fused(s):
            # launch-bound graphs: f-eval (+ masked cotangent), VJP (+ block partials), their reduction - three launches,
            # the same ones the C drivers issue (csrc/small.hip)
            last = pre is not None
            _feval_small(s, t, y_terms, out[0], pre=pre[0] if last else None, alpha=coef if last else 1.0,
                         cot=[(-c, x) for (c, x) in terms[1]], out2=dZ)
            fs = _func_struct(s)
            part = w.small_part(s.groups)
            _vjp_small(s, y_terms, dZ, out[1], part, pre=pre[1] if last else None, out_scale=coef if last else 1.0, fs=fs)
            _finish_small(s, part, packed, t, fs=fs)
            return
        ops.gn_time_gemm(y_terms, n, d, s.groups, s.eps, s.gamma, s.beta, s.W, True, t, out=w.S)
        # k_y = relu(A S + b);  dZ = (-a) * mask
        ops.spmm(s.graph, w.S, bias=s.b, relu=True, out=out[0],
                 cot_terms=[(-c, x) for (c, x) in terms[1]], out2=dZ,
                 pre_terms=pre[0] if pre is not None else None, alpha=coef if pre is not None else 1.0)
        ops.spmm(s.graph.transpose(), dZ, out=dS)                       # dS = A^T dZ
        if ops.bwd_wgrad_supported(n, d, s.groups):
            # large graphs at d = 128: k_a and the weight-gradient partials from ONE read of y and dS (csrc/gemm_pc.hip)
            _, dgp, dbp, part = ops.gn_time_gemm_bwd_wgrad(y_terms, n, d, s.groups, s.eps, s.gamma, s.beta, s.W, True, dS,
                                                           out_scale=coef if pre is not None else 1.0, out=out[1],
                                                           pre_terms=pre[1] if pre is not None else None)
        else:
            _, dgp, dbp = ops.gn_time_gemm_bwd(y_terms, n, d, s.groups, s.eps, s.gamma, s.W, True, dS,
                                               out_scale=coef if pre is not None else 1.0, out=out[1],
                                               pre_terms=pre[1] if pre is not None else None)   # k_a = -a^T df/dy
            part = ops.wgrad(y_terms, n, d, s.groups, s.eps, s.gamma, s.beta, dS, True)
        ops.reduce_parts_(out[3].view(-1), part)                        # row 0 = colsum(dS)
        out[2].copy_((out[3][0] * s.W[0]).sum().reshape(1))             # a_t' = -a^T df/dt
        out[3][0].mul_(t)                                               # dW[0,:] = t * colsum(dS)
        ops.colsum_(out[4], dZ)
        if dgp is not None:
            ops.reduce_parts2_(out[5], dgp, out[6], dbp)
        else:
            out[5].zero_(); out[6].zero_()


class GcnOdePartAdjointField(_PartMixin, GcnOdeAdjointField):
    """Adjoint on a row-partitioned graph: y and a are this rank's rows.  Fixed grid: the small components (a_t and the
    parameter gradients) stay PARTIAL sums over the local rows and the caller sums them over the ranks once per step
    (GradBucket.allreduce_sum) - the adjoint ODE is linear in them, so the sum commutes with the integration.
    Adaptive method: the step-size controller looks at their error norms, so every stage's small derivatives are summed
    over the ranks (one 66 KB all-reduce per stage at d = 128) and every rank integrates the GLOBAL small components;
    param_grads then hands back 1/world of them, so that the caller's allreduce_sum is right in both modes."""
    big_components = (0, 1)

    def _stage(self, t, terms, out, pre, coef):
        GcnOdeAdjointField._stage(self, t, terms, out, pre, coef)
        if self.adaptive and self._part().world > 1:
            packed = getattr(out[2], "_gode_packed", None)
            if packed is not None:
                self.reduce_small(packed)
            else:
                for c in range(2, 7):
                    self.reduce_small(out[c])

    def param_grads(self, comps):
        gs = GcnOdeAdjointField.param_grads(self, comps)
        w = self._part().world
        return [g / w for g in gs] if self.adaptive and w > 1 else gs


class _OdeFuncFn(torch.autograd.Function):
    """Stand-alone differentiable f(t, x) (used when ODEfunc is called outside our solver)."""

    @staticmethod
    def forward(ctx, spec, t, x, W, b, gamma, beta):
        x = x.contiguous()
        n, d = x.shape
        S = ops.gn_time_gemm([(1.0, x)], n, d, spec.groups, spec.eps, gamma, beta, W, True, t)
        out = ops.spmm(spec.graph, S, bias=b, relu=True)
        ctx.spec, ctx.t = spec, t
        ctx.save_for_backward(x, W, b, gamma, beta, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, W, b, gamma, beta, out = ctx.saved_tensors
        spec, t = ctx.spec, ctx.t
        n, d = x.shape
        dZ = g.contiguous() * (out > 0).to(g.dtype)
        dS = ops.spmm(spec.graph.transpose(), dZ)
        dx, dgp, dbp = ops.gn_time_gemm_bwd([(1.0, x)], n, d, spec.groups, spec.eps, gamma, W, True, dS)
        part = ops.wgrad([(1.0, x)], n, d, spec.groups, spec.eps, gamma, beta, dS, True)
        gW = torch.empty_like(W)
        ops.reduce_parts_(gW.view(-1), part)
        gW[0].mul_(t)
        gb = torch.empty_like(b)
        ops.colsum_(gb, dZ)
        gg = torch.zeros_like(gamma)
        gbe = torch.zeros_like(beta)
        if dgp is not None:
            ops.reduce_parts2_(gg, dgp, gbe, dbp)
        return None, None, dx, gW, gb, gg, gbe


def odefunc_apply(adj, t, x, W, b, gamma, beta, groups, eps):
    spec = GcnOdeSpec(as_graph(adj), W, b, gamma, beta, groups, eps)
    return _OdeFuncFn.apply(spec, float(t), x, W, b, gamma, beta)
