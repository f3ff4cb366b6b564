"""Every route and width of the QC edge-message kernels against a float64 restatement: gode_edge_matvec_f32_fwd / _msg_f32 /
_f32_bwd and gode_edge_outer_sum_f32 (csrc/edge.hip), gode_edge_ode_feval_f32 / _feval_save_f32 / _vjp_f32 and
gode_edge_outer_sum_acc_f32 (csrc/edge_ode.hip).

The cases, the limits they bracket and the restatement are in tests/edge_message_routes_design.py; test_edge_message_routes.py
checks on the CPU that every case reaches its routes, that the exact data is exact and the real data well conditioned, the
host-side answers of the entry points, and that nine ways the kernels could be wrong are each rejected by both comparisons
used here.

Every case runs the C ABI itself (outputs pre-filled with NaN, none may remain; strided cases: X / dM / out are column blocks
of NaN-filled matrices with leading dimension h + 3 - dM h + 5 in the outer sum - whose base is not 16-byte aligned, and the
padding of `out` is NaN afterwards) on two kinds of data: `exact` (small integers and powers of two; torch.equal against
float64 rounded to float32) and `real` (the suite's `close` metric against float64: 1e-5 forward, 2e-5 gradients).  A second
run is bit-identical.  The backward runs three times (dA only, dxe only, both: the same bits), the feval in both forms (the
save form's out carries the plain form's bits, k = relu(z)), the VJP by source and by edge (the same dM; every atom and every
edge written).

Routes and the case that reaches each (family/case; test_edge_message_routes.py recomputes them):
  edge_matvec_fwd_kernel<1>                     matvec/width1 .. width256          <16>: width257, width300, wide*
  one tile per edge (h <= 90)                   matvec/width1 .. width90           two: width91, width128, indeg_h91
  three and more tiles                          matvec/width129 (63 + 63 + 3) .. width300, wide2456 (819), wide4096 (2048)
  last tile of one row                          matvec/width91, indeg_h91          short last tile: width129
  T = edges x tiles: 1 / odd / even             matvec/indeg_h16 (in-degrees 1, 3, 255 / 2, 256; 257 and 513 end on T = 1)
  T odd with several tiles                      matvec/width129, width257, wide2457 (two tiles make T even: width91, indeg_h91)
  0 / 1 / 2 / 3 rounds of 256 edges             matvec/indeg_h16, indeg_h91; feval/indeg_h16, indeg_h65 (in-degree 0 .. 513)
  a full last round (256 edges)                 the same four cases
  forward LDS opt-in above 48 KB                matvec/wide2457, wide4096 (exactly 64 KB); just below: wide2456
  lds_dot / column loop: tail only (h < 8)      matvec/width1, width3, width7;  h mod 8 = 0 .. 7: width8, 9, 90, 91, 300, rem5_h13,
                                                rem6_h14, width7
  leading dimensions > h, unaligned base        matvec/strided_h73, strided_h257; outer/strided_t3_h73, strided_t2_h16 (ldx != ldm)
  eid = NULL                                    matvec/eidnull_h16, eidnull_h91; feval/eidnull_h16, eidnull_h65
  val / edge_val = NULL                         matvec/valnull_*, negrow_noval_*; feval/valnull_*; vjp/valnull_h33, negrow_noval_h5
  edge_row = -1                                 matvec/negrow_noval_h9, _h73; outer/negrow_noval_t3_h73; vjp/negrow_h96, negrow_noval_h5
  dA = NULL, dxe = NULL                         every matvec case with a backward
  outer sums, n_terms 1 .. 8                    outer/terms1_h73 .. terms8_h73;  LDS opt-in: terms8_h769, terms8_h1024; below: terms8_h768
  accumulate 0 onto NaN / 1 onto a designed dA  every outer case, weights with a zero and a negative
  feval PF 4 / 16 / 49                          feval/width1 .. width32 / width33 .. width64 / width65 .. width112
  h^2 = 256 PF exactly                          feval/width32, width64, width112;  h mod 4 = 0 .. 3: width4, 5, 110, 3
  feval LDS opt-in (h >= 110)                   feval/width110, width111, width112; just below: width109
  pre with 0 / 1 / 3 / 8 terms x alpha          feval/width* (every pair of them)
  VJP hp 1 .. 128 (G = 256 .. 2)                vjp/width1 (256 groups), width3, width5, width16, width31, width33, width65
  groups without rows / columns without lanes   vjp/width1, width3, width4, width5
  eight-row loop with a tail / without / never  vjp/width33, 65, 109, 110, 111 / width64, 96, 112 / width1 .. width32
  a shorter last group                          vjp/width31, width33, width111
  0 / 1 / 2 / 3 rounds of 16 edges, a full one  vjp/outdeg_h16, _h33, _h65, _h112, eidnull_h16 (out-degrees 0, 1, 15, 16, 17, 33)
  ms_eid = NULL                                 vjp/eidnull_h16, eidnull_h65
  cot with 1 / 3 / 8 terms x cot_scale          vjp/width* (every pair);  fout = +0.0 and -0.0 under the mask: every vjp case
  ops.edge_matvec_fwd at 255 | 256 edges        test_edge_message_across_the_per_edge_threshold
  EdgeOdeField at 4095 | 4096 edges             test_field_across_the_fused_threshold

Measured on an MI355X (worst case of each family; profiles/edge_message_routes_errors.txt has every case; every exact
comparison holds bit for bit):
  edge_matvec fwd / msg       5.5e-7 (out, indeg_h16) / 2.4e-7 (width255);  h > 2048: 7.3e-7 / 6.6e-7 (wide2457)
  edge_matvec bwd             dA 7.6e-8 (indeg_h16), dxe 2.3e-7 (width257);  strided: out 1.8e-7, dxe 3.1e-7 (strided_h257)
  outer sums                  plain 1.5e-7 (terms8_h768), overwriting and accumulating 1.4e-7 (terms8_h769)
  feval, plain and save       out 4.0e-7, k 3.8e-7 (indeg_h65)
  VJP, by source and by edge  dM 1.3e-7 (width96), dS 2.2e-7, dxe 1.4e-7 (width4)
  qc_layers.edge_message      out 8.0e-8 (256 edges), dx 7.2e-8, dA 5.8e-8 (255 edges)
  EdgeOdeField, h = 8         f 4.7e-5, dx 1.2e-4, A 7.9e-5 (4096 edges), W 3.6e-5 (4095 edges): one channel per GroupNorm group, the
                              float32 restatement is as far from float64 and noise_floor_check holds at slack 4

EDGE_MESSAGE_ROUTES_ERRORS=<file>: the errors of the run are written there.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_message_routes_design as D                                  # noqa: E402

pytestmark = pytest.mark.gpu
ERRORS = {}
NAN = float("nan")
ID = lambda c: c.name                                                   # noqa: E731


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def errors_file():
    yield
    path = os.environ.get("EDGE_MESSAGE_ROUTES_ERRORS")
    if path and ERRORS:
        with open(path, "w") as f:
            f.write("# real data: error of every case and quantity against float64, max |got - ref| / max(1, max |ref|)\n")
            f.write("# (bounds 1e-5: out msg k; 2e-5: the rest); the exact data of every case compared equal bit for bit\n")
            for name, errs in ERRORS.items():
                f.write("%-28s %s\n" % (name, " ".join("%s=%.2e" % kv for kv in errs.items())))


def to(t):
    return None if t is None else t.to(dev())


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev())


def block(t, pad):
    """(full, view): t as columns 1 .. 1 + h of a NaN-filled device matrix with h + pad columns, base not 16-byte aligned."""
    full = nan(t.shape[0], t.shape[1] + pad)
    view = full[:, 1:1 + t.shape[1]]
    view.copy_(t)
    assert view.stride() == (t.shape[1] + pad, 1) and view.data_ptr() % 16 != 0
    return full, view


def written(**outs):
    for name, t in outs.items():
        assert not torch.isnan(t).any(), name + ": an element was not written, or a NaN was read"


def padding_is_nan(full, h, what):
    assert torch.isnan(full[:, 0]).all() and torch.isnan(full[:, 1 + h:]).all(), what + ": written outside its columns"


def lib_api():
    from graph_odenet_amd import _lib
    return _lib.load(), _lib.ptr, _lib.check, _lib.stream_ptr


def index_arrays(case):
    b = case.batch
    ix = {k: to(getattr(b, k)) for k in ("src", "tgt", "rowptr", "eid", "ms_rowptr", "ms_eid")}
    assert all(t.dtype == torch.int32 for t in ix.values())
    assert ix["rowptr"].numel() == b.n + 1 == ix["ms_rowptr"].numel() and ix["ms_eid"].numel() == b.E
    return ix


def term_pointers(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for t, x in enumerate(tensors):
        arr[t] = x.data_ptr()
    return arr


# ---- runners: the C ABI on a case's operands ---------------------------------------------------------------------------------
def run_matvec(case, d):
    lib, ptr, check, stream = lib_api()
    b, h, ix = case.batch, case.h, index_arrays(case)
    A, ev = to(d["A"]), to(d["ev"])
    if case.strided:
        (_, X), (_, dM) = block(to(d["X"]), D.PAD), block(to(d["dM"]), D.PAD)
        out_full = nan(b.n, h + D.PAD)
        out = out_full[:, 1:1 + h]
    else:
        X, dM, out = to(d["X"]), to(d["dM"]), nan(b.n, h)
    eid = None if case.sorted_by == "tgt" else ix["eid"]
    val = None if case.noval else ev[ix["eid"].long()].contiguous()
    check(lib.gode_edge_matvec_f32_fwd(ptr(ix["rowptr"]), ptr(eid), ptr(val), ptr(ix["src"]), ptr(A), ptr(X), X.stride(0), h, b.n,
                                       ptr(out), out.stride(0), stream()), "gode_edge_matvec_f32_fwd")
    msg = nan(b.E, h)
    check(lib.gode_edge_matvec_msg_f32(ptr(ix["src"]), ptr(A), ptr(X), X.stride(0), h, b.E, ptr(msg), stream()), "gode_edge_matvec_msg_f32")
    written(out=out, msg=msg)
    res = {"out": out, "msg": msg}
    if case.strided:
        padding_is_nan(out_full, h, "out")
    if case.fwd_only:
        return res
    edge_val = None if case.noval else ev
    for want_dA, want_dx in ((True, False), (False, True), (True, True)):
        dA, dxe = (nan(b.E, h, h) if want_dA else None), (nan(b.E, h) if want_dx else None)
        check(lib.gode_edge_matvec_f32_bwd(ptr(ix["tgt"]), ptr(edge_val), ptr(ix["src"]), ptr(A), ptr(X), X.stride(0), ptr(dM),
                                           dM.stride(0), h, b.E, ptr(dA), ptr(dxe), stream()), "gode_edge_matvec_f32_bwd")
        if want_dA and want_dx:
            assert torch.equal(dA, res["dA"]) and torch.equal(dxe, res["dxe"]), "dA / dxe depend on which of them is asked for"
        if want_dA:
            res["dA"] = dA
        if want_dx:
            res["dxe"] = dxe
    written(dA=res["dA"], dxe=res["dxe"])
    return res


def run_outer(case, d):
    lib, ptr, check, stream = lib_api()
    b, h, ix, n = case.batch, case.h, index_arrays(case), case.n_terms
    edge_val = None if case.noval else to(d["ev"])
    dMs_c, Xs_c = [to(t) for t in d["dMs"]], [to(t) for t in d["Xs"]]
    if case.strided:                                  # ldx = h + 3, ldm = h + 5
        dMs, Xs = [block(t, D.PAD + 2)[1] for t in dMs_c], [block(t, D.PAD)[1] for t in Xs_c]
        assert Xs[0].stride(0) != dMs[0].stride(0)
    else:
        dMs, Xs = dMs_c, Xs_c
    plain = nan(b.E, h, h)
    check(lib.gode_edge_outer_sum_f32(ptr(ix["tgt"]), ptr(edge_val), ptr(ix["src"]), n, term_pointers(dMs), term_pointers(Xs),
                                      Xs[0].stride(0), dMs[0].stride(0), h, b.E, ptr(plain), stream()), "gode_edge_outer_sum_f32")
    ws = (ctypes.c_float * n)(*d["w"])
    over, acc = nan(b.E, h, h), to(d["dA0"]).clone()
    for accumulate, dA in ((0, over), (1, acc)):
        check(lib.gode_edge_outer_sum_acc_f32(ptr(ix["tgt"]), ptr(edge_val), ptr(ix["src"]), n, term_pointers(dMs_c), term_pointers(Xs_c),
                                              ws, h, b.E, accumulate, ptr(dA), stream()), "gode_edge_outer_sum_acc_f32")
    written(plain=plain, over=over, acc=acc)
    return {"plain": plain, "over": over, "acc": acc}


def run_feval(case, d):
    from graph_odenet_amd import _lib
    lib, ptr, check, stream = lib_api()
    b, h, ix = case.batch, case.h, index_arrays(case)
    A, S, bias, pre = to(d["A"]), to(d["X"]), to(d["bias"]), [to(t) for t in d["pre"]]
    eid = None if case.sorted_by == "tgt" else ix["eid"]
    val = None if case.noval else to(d["ev"])[ix["eid"].long()].contiguous()
    lc = _lib.lincomb(list(zip(d["coef"], pre))) if pre else None
    lcp = ctypes.byref(lc) if lc is not None else None
    out, out_save, k = nan(b.n, h), nan(b.n, h), nan(b.n, h)
    check(lib.gode_edge_ode_feval_f32(ptr(ix["rowptr"]), ptr(eid), ptr(val), ptr(ix["src"]), ptr(A), ptr(S), h, b.n, ptr(bias), lcp,
                                      case.alpha, ptr(out), stream()), "gode_edge_ode_feval_f32")
    check(lib.gode_edge_ode_feval_save_f32(ptr(ix["rowptr"]), ptr(eid), ptr(val), ptr(ix["src"]), ptr(A), ptr(S), h, b.n, ptr(bias), lcp,
                                           case.alpha, ptr(out_save), ptr(k), stream()), "gode_edge_ode_feval_save_f32")
    written(out=out, out_save=out_save, k=k)
    assert torch.equal(out, out_save), "the save form's out differs from the plain form's"
    assert k.min().item() >= 0.0
    return {"out": out, "k": k}


def run_vjp(case, d):
    from graph_odenet_amd import _lib
    lib, ptr, check, stream = lib_api()
    b, h, ix = case.batch, case.h, index_arrays(case)
    A, fout, cot = to(d["A"]), to(d["fout"]), [to(t) for t in d["cot"]]
    edge_val = None if case.noval else to(d["ev"])
    ms_eid = None if case.sorted_by == "src" else ix["ms_eid"]
    lc = _lib.lincomb(list(zip(d["coef"], cot)))
    dM, dS, dM_e, dxe = nan(b.n, h), nan(b.n, h), nan(b.n, h), nan(b.E, h)
    check(lib.gode_edge_ode_vjp_f32(ptr(ix["ms_rowptr"]), ptr(ms_eid), ptr(ix["tgt"]), ptr(edge_val), ptr(A), ctypes.byref(lc),
                                    case.cot_scale, ptr(fout), h, b.n, b.E, ptr(dM), ptr(dS), None, stream()), "gode_edge_ode_vjp_f32 by source")
    check(lib.gode_edge_ode_vjp_f32(None, None, ptr(ix["tgt"]), ptr(edge_val), ptr(A), ctypes.byref(lc), case.cot_scale, ptr(fout), h,
                                    b.n, b.E, ptr(dM_e), None, ptr(dxe), stream()), "gode_edge_ode_vjp_f32 by edge")
    written(dM=dM, dS=dS, dM_by_edge=dM_e, dxe=dxe)             # every atom's dM and every edge's dxe in the by-edge form too
    assert torch.equal(dM, dM_e), "dM differs between the two forms"
    return {"dM": dM, "dS": dS, "dxe": dxe}


RUNNERS = {"matvec": run_matvec, "outer": run_outer, "feval": run_feval, "vjp": run_vjp}


def run_case(case):
    run = RUNNERS[case.family]
    for kind in ("exact", "real"):
        d = D.inputs(case, kind)
        ref = D.reference(case, d)
        got = run(case, d)
        assert set(got) == set(ref)
        if kind == "exact":
            bad = D.unequal(got, ref)
            print("%s/%s exact: %s" % (case.family, case.name, "equal" if not bad else "UNEQUAL " + ", ".join(bad)))
            assert not bad, "%s/%s: not the float64 result on the exact data: %s" % (case.family, case.name, ", ".join(
                "%s (err %.3e)" % (k, D.rel_err(got[k], ref[k])) for k in bad))
        else:
            errs = D.errors(got, ref)
            ERRORS["%s/%s" % (case.family, case.name)] = errs
            print("%s/%s real: %s" % (case.family, case.name, " ".join("%s=%.2e" % kv for kv in errs.items())))
            bad = D.failures(errs)
            assert not bad, "%s/%s: %s" % (case.family, case.name, ", ".join("%s %.3e > %.1e" % (k, errs[k], D.tolerance(k)) for k in bad))
        if case.negrows:
            dead = to(case.batch.tgt < 0)
            for k in ("dA", "dxe", "plain", "over"):                 # an edge without a target: exactly zero, whatever dM holds
                if k in got:
                    assert got[k][dead].abs().max().item() == 0.0, k
            if "acc" in got:
                assert torch.equal(got["acc"][dead], to(d["dA0"])[dead])
        again = run(case, d)                                         # fixed summation order: bit-identical
        for k, t in got.items():
            assert torch.equal(t, again[k]), k + " differs between two runs"


@pytest.mark.parametrize("case", D.MATVEC_CASES, ids=ID)
def test_edge_matvec_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.OUTER_CASES, ids=ID)
def test_edge_outer_sums_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.FEVAL_CASES, ids=ID)
def test_edge_ode_feval_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.VJP_CASES, ids=ID)
def test_edge_ode_vjp_vs_float64(case):
    run_case(case)


# ---- through the public functions --------------------------------------------------------------------------------------------
def random_batch(n, E, h, seed):
    g = torch.Generator().manual_seed(seed)
    src, tgt = torch.randint(0, n, (E,), generator=g), torch.randint(0, n - 1, (E,), generator=g)     # the last atom receives nothing
    val = torch.rand(E, generator=g) + 0.5
    A = torch.randn(E, h, h, generator=g) / h ** 0.5
    x = torch.randn(n, h, generator=g)
    return src, tgt, val, A, x, g


@pytest.mark.parametrize("E", D.PUBLIC_MESSAGE_EDGES)
def test_edge_message_across_the_per_edge_threshold(E):
    """qc_layers.edge_message forward and backward at h = 9 with 255 edges (one launch over the targets) and 256 (a workgroup per
    edge + SpMM), against float64."""
    from graph_odenet_amd import ops, qc_layers
    n, h = 30, 9
    assert ops.EDGE_MSG_MIN_EDGES == D.EDGE_MSG_MIN_EDGES
    src, tgt, val, A, x, g = random_batch(n, E, h, 40 + E)
    gout = torch.randn(n, h, generator=g)
    xr, Ar = x.double().requires_grad_(True), A.double().requires_grad_(True)
    ref = torch.zeros(n, h, dtype=torch.float64).index_add(0, tgt, val.double()[:, None] * torch.bmm(Ar, xr[src].unsqueeze(2)).squeeze(2))
    ref.backward(gout.double())
    xd, Ad = to(x).requires_grad_(True), to(A).requires_grad_(True)
    out = qc_layers.edge_message(xd, to(src), qc_layers.prepared_edges(to(src), to(tgt), n, to(val)), Ad)
    out.backward(to(gout))
    errs = {"out": D.rel_err(out, ref), "dx": D.rel_err(xd.grad, xr.grad), "dA": D.rel_err(Ad.grad, Ar.grad)}
    ERRORS["public/edge_message_E%d" % E] = errs
    print("edge_message E=%d: %s" % (E, " ".join("%s=%.2e" % kv for kv in errs.items())))
    assert not D.failures(errs), errs


@pytest.mark.parametrize("E", D.PUBLIC_FIELD_EDGES)
def test_field_across_the_fused_threshold(E):
    """One EdgeOdeField evaluation and VJP at h = 8 with 4095 edges (fused: one launch each) and 4096 (per edge), with the
    helpers and to the bar of test_gpu_qc_ode.py: noise_floor_check with slack_of(h)."""
    import test_gpu_qc_ode as Q
    from graph_odenet_amd import ops
    n, h, t = 400, 8, 0.375
    assert ops.EDGE_ODE_FUSED_MAX_EDGES == D.EDGE_ODE_FUSED_MAX_EDGES
    Esrc, etgt, val, A, x0, g = random_batch(n, E, h, 50 + E)
    etgt[0] = n - 2                                               # Q.product sizes the batch as max target + 2
    A = A * 0.5
    a = torch.randn(n, h, generator=g)
    f, Ad = Q.product(h, Esrc, etgt, val, A)
    fwd, mk_adj, plist = f.gode_fields(to(x0))
    x, ad = to(x0), to(a)
    out = torch.empty_like(x)
    with Q.profiled() as kinds:
        fwd.eval(t, [[(1.0, x)]], [out])
    assert kinds.count(ops.PROF_EDGE_FEVAL) == (1 if E < ops.EDGE_ODE_FUSED_MAX_EDGES else 0)
    adj = mk_adj()
    state = adj.new_state(x)
    k = adj.alloc_like(state, 1)[0]
    adj.eval(t, [[(1.0, x)], [(1.0, ad)], [(1.0, state[2])], [(1.0, state[3])], [(1.0, state[4])]], k)
    v = adj.s.views(k[3])
    got = {"f": out, "fy": k[0], "dx": k[1], "a_t": k[2], "gamma": v["gamma"], "beta": v["beta"], "W": v["W"], "b": v["b"], "A": k[4]}
    want = []
    for ref in Q.ref_pair(f, h, Esrc, etgt, val, A):
        dt = ref.W.dtype
        tt = torch.tensor(t, dtype=dt, requires_grad=True)
        xr = x0.detach().clone().to(dt).requires_grad_(True)
        fe = ref(tt, xr)
        gr = torch.autograd.grad(fe, (tt, xr, ref.gamma, ref.beta, ref.W, ref.b, ref.A), -a.to(dt))
        want.append(dict(zip(("f", "fy", "a_t", "dx", "gamma", "beta", "W", "b", "A"), (fe.detach(), fe.detach()) + gr)))
    ERRORS["public/field_E%d" % E] = {key: D.rel_err(got[key].reshape(want[1][key].shape), want[1][key]) for key in got}
    print("field E=%d: %s" % (E, " ".join("%s=%.2e" % kv for kv in ERRORS["public/field_E%d" % E].items())))
    for key in got:
        Q.noise_floor_check(got[key].reshape(want[1][key].shape), want[0][key], want[1][key], "E=%d %s" % (E, key), slack=Q.slack_of(h))


def test_edge_ode_supported_widths():
    from graph_odenet_amd import ops
    assert ops.edge_ode_supported(D.ODE_HMAX) and D.ODE_HMAX == 112
    assert not ops.edge_ode_supported(113) and not ops.edge_ode_supported(0)
