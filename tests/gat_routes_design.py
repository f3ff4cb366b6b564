"""Designed inputs and the float64 restatement for the edge-attention route tests (test_gat_routes.py checks the design's
conditions on the CPU, test_gpu_gat_routes.py runs the kernels on it).  numpy / CPU torch only; nothing of the library and
nothing of oracle/ is used here.

Graphs.  S has 701 rows, L has 66 003 (more than 65 536; neither is a multiple of 4 or 16, the rows per block of the
prefetched kernels).  Rows of every degree the loops branch on (SHORT: the prefetched kernels' chunk of 16 / 64 slots and
their 1..16 edges per trip, the wave kernels' stride 64 / G, the record kernels' lane-group chunk and 4-way unroll) and
rows that the record list splits at SPLIT = 96 into 2, 3, 4, 5, 9 and 11 slots (LONG) sit at chosen rows - row 0, the last
row and, in L, rows 65 535 and 65 536 included - each beside an empty row; the rest of S, and about 3 000 rows of L, have
1..3 edges, every other row of L is empty (E stays near 12 000).  A few rows repeat a source node.  Edge values are
multiples of 1/4 in 0.5..1.5, or absent (pattern only).  The non-canonical variant lists the edges in a shuffled order
and gives a tenth of the edges of short rows a `tgt` that is not their row of Mtgt.  B0 / B1 have 65 536 / 65 537 rows, all
busy (the two sides of the row threshold).

Values.  Ps, Pt, bf, dout and the cotangent terms are multiples of 1/4 in [-2, 2], coefficients and cot_scale signed powers
of two: z = Ps[src] + Pt[tgt] + bf and the combined cotangent are exact fp32 numbers whatever the order of the sums, and
z == 0 on about 4 % of the entries (`>` against `>=` in the relu mask of dz).  A2 is uniform in [-1, 1], bw = 0.375.

Node arrays are kept COMPACT over the active nodes (`act`: every node that has an edge, as source, target or row): the
inactive rows of L are never read by a kernel, and must be written as zeros (checked on the GPU side).
"""
import functools

import numpy as np
import torch

SPLIT = 96
SHORT = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]
LONG = [192, 193, 288, 384, 389, 480, 769, 863, 1000]
SLOT_COUNTS = {2, 3, 4, 5, 9, 11}
N_OF = {"S": 701, "L": 66_003, "B0": 65_536, "B1": 65_537}      # B0 / B1: the two sides of the row threshold, every row busy
THRESHOLD = 65_536
EPS = 1e-9
BW = 0.375
MAX_TERMS = 8
MIN_SHARE = 1e-4
TOL = 2e-5


class Design:
    pass


@functools.lru_cache(maxsize=None)
def design(kind, canonical=True, pattern=False):
    """The designed graph.  src / tgt: the edge list as handed to EdgeGraph; rows / cols / vals: the entries of Mtgt
    (entry k = (rows[k], edge cols[k], vals[k]), sorted by row, then edge id)."""
    n = N_OF[kind]
    rs = np.random.RandomState(7 + n)
    special = [1000] + SHORT + [x for x in LONG if x not in (1000, 863)] + [863]
    if kind != "L":
        pos = np.round(np.linspace(0, n - 1, len(special))).astype(np.int64)
    else:
        k = len(special)
        below = np.round(np.linspace(0, THRESHOLD - 300, k - 8)).astype(np.int64)
        pos = np.concatenate([below, [THRESHOLD - 1, THRESHOLD], np.round(np.linspace(THRESHOLD + 4, n - 1, 6)).astype(np.int64)])
    assert len(set(pos.tolist())) == len(special) and pos[0] == 0 and pos[-1] == n - 1
    deg = np.zeros(n, np.int64)
    if kind != "L":
        deg[:] = rs.randint(1, 4, n)
    else:
        bulk = np.concatenate([rs.choice(THRESHOLD - 2, 2600, replace=False), np.arange(THRESHOLD + 2, n)])
        deg[bulk] = rs.randint(1, 4, bulk.size)
    spec = {}
    for p in pos:                                       # an empty row beside every special row
        for q in (p + 1, p - 1):
            if 0 <= q < n and q not in pos:
                deg[q] = 0
                break
    for p, s in zip(pos, special):
        deg[p] = s
        spec[int(p)] = s
    if kind == "L":
        assert deg[THRESHOLD - 2] == 0 and deg[THRESHOLD + 1] == 0
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    E = int(rowptr[-1])
    tgt = np.repeat(np.arange(n), deg)
    pool = np.arange(n) if kind != "L" else np.unique(np.concatenate(
        [rs.choice(n, 1500, replace=False), [0, n - 1, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1]]))
    src = pool[rs.randint(0, pool.size, E)]
    src[0], src[E - 1] = 0, n - 1
    repeated = []
    for p, s in spec.items():                           # one source node repeated within a row
        if s in (2, 5, 64, 193, 1000):
            src[rowptr[p] + 1] = src[rowptr[p]]
            repeated.append(p)
    vals = (rs.randint(2, 7, E) / 4.0).astype(np.float32)
    d = Design()
    d.kind, d.n, d.E, d.canonical, d.pattern = kind, n, E, canonical, pattern
    d.special, d.repeated, d.deg = spec, repeated, deg
    if canonical:
        d.src, d.tgt = src, tgt
        d.rows, d.cols = tgt.copy(), np.arange(E)
    else:
        perm = rs.permutation(E)                        # entry k of the sorted list is edge perm[k]
        order = np.lexsort((perm, tgt))                 # entries sorted by row, then edge id
        d.rows, d.cols = tgt[order], perm[order]
        vals = vals[order]
        e_src, e_tgt = np.empty(E, np.int64), np.empty(E, np.int64)
        e_src[perm], e_tgt[perm] = src, tgt
        short = np.flatnonzero((deg[e_tgt] <= 16) & (rs.randint(0, 10, E) == 0))
        e_tgt[short] = pool[rs.randint(0, pool.size, short.size)]
        d.src, d.tgt = e_src, e_tgt
    d.vals = None if pattern else vals
    d.act = np.unique(np.concatenate([d.src, d.tgt, d.rows]))
    lut = np.full(n, -1, np.int64)
    lut[d.act] = np.arange(d.act.size)
    d.lut = lut
    return d


def slot_counts(deg, split=SPLIT):
    return {int(-(-x // split)) for x in deg if x > split}


def quarters(rs, *shape):
    return (rs.randint(-8, 9, shape) / 4.0).astype(np.float32)


@functools.lru_cache(maxsize=4)
def values(kind, canonical, o):
    """Compact node arrays (len(act) rows) of one case, as CPU float32 tensors."""
    d = design(kind, canonical)
    rs = np.random.RandomState(1000 * o + d.n % 1000)
    na = d.act.size
    v = Design()
    v.Ps, v.Pt, v.dout = (torch.from_numpy(quarters(rs, na, o)) for _ in range(3))
    v.bf = torch.from_numpy(quarters(rs, o))
    v.A2 = torch.from_numpy(rs.uniform(-1.0, 1.0, (na, 2)).astype(np.float32))
    v.bw = torch.tensor([BW], dtype=torch.float32)
    v.cot = [torch.from_numpy(quarters(rs, na, o)) for _ in range(MAX_TERMS)]
    v.coef = [float(s * 2.0 ** p) for s, p in zip((1, -1, 1, 1, -1, -1, 1, -1), (0, -1, 1, -1, 0, 1, -1, 0))]
    v.cot_scale = -0.5
    return v


def logits32(d, v):
    """a and its maximum exactly as the kernels form them: fp32 (as[src] + at[tgt]) + bw."""
    s, t = torch.from_numpy(d.lut[d.src]), torch.from_numpy(d.lut[d.tgt])
    a = (v.A2[s, 0] + v.A2[t, 1]) + v.bw[0]
    return a, a.max()


FAULTS = ("bias_first_chunk_only", "no_val_in_backward", "mask_ge", "finish_one_slot_early", "no_cot_scale")


def reference(d, v, n_terms=0, fault=None):
    """float64 restatement over the compact nodes, with index_add only.  n_terms == 0: the cotangent is dout; else it is
    cot_scale * sum_j coef_j cot_j masked by out > 0.  da / dA2 come WITHOUT the path through the maximum.
    fault (one of FAULTS): the same arithmetic wrong in one way a kernel could be wrong - the bias reaching only the first
    64 columns of the forward, val missing from the backward, `>=` for `>` in the relu mask, the finishing launches of the
    record route leaving out each split row's last slot, cot_scale missing.  test_gat_routes.py holds these against the
    reference under the GPU tests' metric and bound: each must be rejected."""
    assert fault is None or fault in FAULTS
    f64 = torch.float64
    s, t = torch.from_numpy(d.lut[d.src]), torch.from_numpy(d.lut[d.tgt])
    r, c = torch.from_numpy(d.lut[d.rows]), torch.from_numpy(d.cols)
    na, o = v.Ps.shape
    val = torch.ones(d.E, dtype=f64) if d.vals is None else torch.from_numpy(d.vals).to(f64)
    a32, amax = logits32(d, v)
    w = torch.exp(a32.to(f64) - amax.to(f64))                                  # per edge
    z = (v.Ps[s] + v.Pt[t]).to(f64) + v.bf.to(f64)                             # gathered in fp32 (exact), then double
    y = torch.clamp(z, min=0.0)
    y_fwd = y
    if fault == "bias_first_chunk_only":
        y_fwd = torch.clamp(z - torch.where(torch.arange(o) >= 64, v.bf.to(f64), torch.zeros(o, dtype=f64)), min=0.0)
    we = val * w[c]                                                            # per entry of Mtgt
    closed = torch.ones(d.E, dtype=f64)                                        # entries the row's closing sum includes
    if fault == "finish_one_slot_early":
        first = np.zeros(d.n + 1, np.int64)
        first[1:] = np.cumsum(np.bincount(d.rows, minlength=d.n))
        k, deg = np.arange(d.E) - first[d.rows], (first[1:] - first[:-1])[d.rows]
        closed = torch.from_numpy(((deg <= SPLIT) | (k < (-(-deg // SPLIT) - 1) * SPLIT)).astype(np.float64))
    ssum = torch.zeros(na, dtype=f64).index_add_(0, r, we * closed)
    den = ssum + EPS
    num = torch.zeros(na, o, dtype=f64).index_add_(0, r, (we * closed)[:, None] * y_fwd[c])
    out = num / den[:, None]
    if n_terms:
        g = sum(cf * ct.to(f64) for cf, ct in zip(v.coef[:n_terms], v.cot[:n_terms]))
        g = g * (1.0 if fault == "no_cot_scale" else v.cot_scale)
        g = torch.where(out > 0, g, torch.zeros_like(g))
    else:
        g = v.dout.to(f64)
    dA = g / den[:, None]
    dsum = -(g * out).sum(1) / den
    web = w[c] if fault == "no_val_in_backward" else we
    dz = torch.zeros(d.E, o, dtype=f64)
    dz[c] = web[:, None] * dA[r] * ((z[c] >= 0) if fault == "mask_ge" else (z[c] > 0)).to(f64)
    da = torch.zeros(d.E, dtype=f64)
    da[c] = web * ((dA[r] * y[c]).sum(1) + dsum[r])
    mag = torch.zeros(d.E, dtype=f64)                                          # da without its cancellation
    mag[c] = we * ((dA[r] * y[c]).abs().sum(1) + dsum[r].abs())
    ref = Design()
    ref.a32, ref.amax, ref.w, ref.den, ref.out, ref.dz, ref.da, ref.mag = a32, amax, w, den, out, dz, da, mag
    ref.share = we / den[r]
    ref.z = z
    ref.dPs = torch.zeros(na, o, dtype=f64).index_add_(0, s, dz)
    ce = torch.ones(d.E, dtype=f64)
    ce[c] = closed                                                             # per edge
    ref.dPt = torch.zeros(na, o, dtype=f64).index_add_(0, t, dz * ce[:, None])
    ref.dA2 = torch.stack([torch.zeros(na, dtype=f64).index_add_(0, s, da), torch.zeros(na, dtype=f64).index_add_(0, t, da * ce)], 1)
    ref.magA2 = torch.stack([torch.zeros(na, dtype=f64).index_add_(0, s, mag), torch.zeros(na, dtype=f64).index_add_(0, t, mag)], 1)
    ref.magPs = torch.zeros(na, o, dtype=f64).index_add_(0, s, dz.abs())       # the node sums of dz without their cancellation
    ref.magPt = torch.zeros(na, o, dtype=f64).index_add_(0, t, dz.abs())
    ref.edge_row = torch.empty(d.E, dtype=torch.int64)
    ref.edge_row[c] = r                                                        # the row of Mtgt an edge is summed into
    return ref


# ---- the metric: errors relative to the ROW's own scale ------------------------------------------------------------------
def row_max(x, row, n_rows):
    """max |x| over the entries (all columns) that belong to each row."""
    x = x.abs().reshape(x.shape[0], -1).max(1).values.numpy()
    m = np.zeros(n_rows)
    np.maximum.at(m, row.numpy(), x)
    return torch.from_numpy(m)


def scaled_error(got, ref, scale):
    """max over rows of |got - ref| / scale[row], and whether every entry with scale 0 is exactly 0 in `got`.
    got / ref: [rows, ...]; scale: [rows]."""
    got, ref = got.to(torch.float64).reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    zero = scale == 0
    exact = bool((got[zero] == 0).all())
    live = ~zero
    if not live.any():
        return 0.0, exact
    err = ((got[live] - ref[live]).abs() / scale[live][:, None]).max().item()
    return err, exact


def edge_error(got, ref, edge_row, n_rows, scale_src=None):
    """Per-edge array: the scale of an edge is the largest |scale_src| (default: |ref|) among the edges of its row."""
    m = row_max(ref if scale_src is None else scale_src, edge_row, n_rows)
    return scaled_error(got, ref, m[edge_row])


CANCEL_FLOOR = 1.0 / 16


def node_error(got, ref, scale_src=None, terms_mag=None):
    """Per-node array: the scale of a row is its own largest |scale_src| (default: |ref|).  terms_mag (for a node sum: the
    sum of the absolute values of its terms): a row that cancelled below CANCEL_FLOOR of its terms is measured against that
    fraction of them.  The terms are themselves only right to a few 1e-7 of their size, so a sum that cancelled to 1/1000
    of them carries 1e-4 of its own size in rounding error whatever computes it: at o = 1 a plain fp32 restatement of the
    reference is 4.3e-4 away under the unfloored metric (2e-5 at o = 2, 2e-6 from o = 7 on, where no row of the designed
    graphs cancels below 1/30 and the floor at most doubles a hub row's scale)."""
    src = ref if scale_src is None else scale_src
    scale = src.abs().reshape(src.shape[0], -1).max(1).values
    if terms_mag is not None:
        scale = torch.maximum(scale, CANCEL_FLOOR * terms_mag.reshape(terms_mag.shape[0], -1).max(1).values)
    return scaled_error(got, ref, scale)


def compare_forward(ref, w, den, out):
    """{quantity: (error, zero rows exact)} of a forward's results (compact rows, CPU) against the reference."""
    na = ref.den.shape[0]
    return {"w": edge_error(w, ref.w, ref.edge_row, na), "den": node_error(den, ref.den), "out": node_error(out, ref.out)}


def compare_backward(ref, dz, da, dPs, dPt, dA2):
    na = ref.den.shape[0]
    return {"dz": edge_error(dz, ref.dz, ref.edge_row, na),
            "da": edge_error(da, ref.da, ref.edge_row, na, scale_src=ref.mag),
            "dPs": node_error(dPs, ref.dPs, terms_mag=ref.magPs), "dPt": node_error(dPt, ref.dPt, terms_mag=ref.magPt),
            "dA2": node_error(dA2, ref.dA2, scale_src=ref.magA2)}


def passes(result):
    return all(err <= TOL and exact for err, exact in result.values())
