"""Every route of the Runge-Kutta vector and reduction kernels (csrc/rk.hip) against float64: gode_lincomb_f32,
gode_lincomb_multi_f32, gode_rk_errnorm_f32, gode_rk_errnorm_multi_f32, gode_rk_scaled_sumsq_f32, gode_reduce_parts_f32,
gode_reduce_parts2_f32, gode_reduce_segments_f32, gode_colsum_f32 and gode_colsum_parts_f32.

The cases, the limits they bracket, the float64 reference and the derived bounds are in tests/rk_routes_design.py;
test_rk_routes.py checks on the CPU that every case reaches its routes, that the exact data is exact and plain float32 stays
inside the bounds on the real data, the host-side answers of the entry points, and that fifteen ways the kernels could be
wrong are each rejected by both comparisons used here.

Every case drives the C ABI itself.  Every operand is a view into a NaN-filled buffer eight floats longer than it (a
misaligned operand starts one float into its buffer: data_ptr() % 16 != 0 is asserted); no NaN may remain inside the written
length, and every float outside it is NaN afterwards.  Each case runs on two kinds of data: `exact` (np.array_equal against
float64 rounded to float32; == on the float64 error sums) and `real` (elementwise inside the derived bound).  A second run is
bit-identical (no kernel here uses atomics).  Every output and sum of a multi form is the single form's bit for bit, and
inside its float64 bound too.

Routes and the cases that reach them (family/case; test_rk_routes.py recomputes them):
  lincomb4_kernel / lincomb1_kernel             lincomb/n4, n256, n1024, n1028 / n1, n3, n5, n255, n257, n1023
  grid-stride wrap (8192 blocks)                lincomb/wrap4 (n = 8 388 612, one trailing float4) / wrap1 (n = 2 097 153)
  1 .. 8 terms in each form                     lincomb/terms1_n1028 .. terms8_n1028 / terms1_n1023 .. terms8_n1023
  in place on term 0 / on the last term         lincomb/inplace0_n1028, inplace0_n257 / inplacelast_n1028, inplacelast_n257
  out / the last term / every operand misaligned lincomb/mis_out_n1028 / mis_last_n1028 / mis_all_n1028, mis_all_n257
  lincomb_multi_kernel, count 1 .. 4            lincomb_multi/count1 .. count4, count4_scalar: both forms in one launch, lengths
                                                1 and 1028 together, ns[1] = 0 in the middle (stays NaN), one component in place
  ratio_sumsq4_kernel<0 | 1> / ratio_sumsq_kernel err/n4, n1024, n1028, n4096 / n1, n3, n1023, n1025 (each _m0 and _m1)
  1024 blocks: full / wrapping                  err/full (n = 1 048 576) / wrap4 (1 048 580), wrap1 (1 048 577, scalar)
  1 .. 8 terms in each form and mode            err/terms1_n1028 .. terms8_n1028 / terms1_n1025 .. terms8_n1025
  y0 / y1 / one term misaligned                 err/mis_y0_n1028 / mis_y1_n1028_m0 / mis_term_n1028
  rtol = 0 / atol = 0                           err/rtol0_n1028, rtol0_n1025 / atol0_n1028, atol0_n1025
  one live element: the sum is its ratio squared err/plant<i>_n<n>: first, last, either side of the last whole float4, of a block
                                                boundary and of the wrap (design: PLANTS)
  ratio_sumsq_multi_kernel, count 1 .. 4        err_multi/count1 .. count4, count3, count3_mixed (lengths 1 and 1 048 580: nb 1 and 1024)
  reduce_parts_kernel: tail only / four loads   parts/1x33, 7x31, 8x32, 9x1, 9x33, 24x33 / 25x33 .. 63x4096, 128x1000, 512x33
  stays scalar at the 16-byte form's edge       parts/63x4096, 64x4097, 64x4092, 64x4096 with out misaligned
  reduce_parts4_kernel                          parts/64x4096, 64x4100 (partly filled last block), 65 .. 113 (tails), 128, 512 x 4096
  no partials / accumulate / scale 1, -0.5, 0   parts/0x33, 0x32 / every second case onto a designed vector, else onto NaN
  gode_reduce_parts2_f32                        parts2/37x33, 9x1: two pairs with different data
  reduce_segments_kernel                        segs/one, eight (strides 2 and 3, col0, ld surplus, at = NULL), time_one, time_two
                                                (two time segments, time_len 33 = two trips, time_len < len, a weight row with
                                                time_len 0), wrow_without_time
  colsum4_kernel                                colsum/257x4, 513x12, 256x128, 0x128, 1x128, 255x300, 2x300, 4097x1024, 2049x512
  1024 blocks, the last two past the end        colsum/262400x4
  colsum_kernel, d <= 256                       colsum/513x1, 257x3, 0x3, 256x7, 1x7, 255x73, 2x255, 513x256 and 257x12 with X misaligned
  colsum_kernel, d > 256                        colsum/513x257, 257x301, 255x511, 2053x513, 4113x1028
  colsum_wide_kernel                            colsum/2048x512 (2049x512: the row blocks), {0, 1, 7, 8, 9, 63, 64, 65, 127, 128} x {513, 2667}
  the ops wrappers                              test_ops_wrappers

Measured on an MI355X (real data, worst case of each entry point: the suite's metric max |got - ref| / max(1, max |ref|), and
the largest fraction of the derived bound any element used; profiles/rk_routes_errors.txt has every case; every exact
comparison held bit for bit):
  gode_lincomb_f32              1.2e-7 (terms6_n1023); 0.65 of the bound (wrap1), 0.50 (wrap4)
  gode_lincomb_multi_f32        4.1e-7 (count4_scalar[2]); 0.62 of the bound (count4_scalar[1])
  gode_rk_errnorm_f32           1.8e-7, 0.21 of the bound (n1_m0); the 2^20-element sums 1.9e-11 (wrap4_m0)
  gode_rk_scaled_sumsq_f32      1.7e-7, 0.23 of the bound (plant0_n1025_m1); 2.9e-10 (wrap1_m1)
  gode_rk_errnorm_multi_f32     9.5e-8, 0.07 of the bound (count4[2])
  gode_reduce_parts_f32         1.9e-7 (113x4100_acc1_scale1); 0.45 of the bound (1x33_acc1_scale1)
  gode_reduce_parts2_f32        1.3e-7 (37x33_acc0_scale1); 0.04 of the bound (9x1_acc1_scale-0.5)
  gode_reduce_segments_f32      outputs 1.5e-7, 0.18 of the bound (eight); at 5.7e-7, 0.002 of the bound (time_one)
  gode_colsum_f32               4.7e-7 (255x511_acc1_scale1); 0.67 of the bound (2x300_acc1_scale-0.5)
  gode_colsum_parts_f32         5.5e-7 (2053x513_acc0_scale-0.5); 0.33 of the bound (2x300_acc1_scale-0.5)
  the ops wrappers              4.8e-7 (colsum_parts, 257x301); 0.55 of the bound (lincomb_, n1028)
The float32 division of the error ratios is correctly rounded on the exact operands: all 103 exact error sums (and the 12 of
the multi form) compare == .

RK_ROUTES_ERRORS=<file>: the figures of the run are written there.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rk_routes_design as D                                            # noqa: E402

pytestmark = pytest.mark.gpu
ERRORS = {}
NAN = float("nan")
PAD = 8
ID = lambda c: c.name                                                   # noqa: E731


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def errors_file():
    yield
    path = os.environ.get("RK_ROUTES_ERRORS")
    if path and ERRORS:
        with open(path, "w") as f:
            f.write("# real data, every case and quantity against float64: max |got - ref| / max(1, max |ref|), and the largest\n")
            f.write("# fraction of the derived bound (tests/rk_routes_design.py) any element used; the exact data of every case\n")
            f.write("# compared equal bit for bit\n")
            for name, figs in ERRORS.items():
                f.write("%-44s %s\n" % (name, "  ".join("%s=%.2e (%.3f of bound)" % (k, m, fr) for k, (m, fr) in figs.items())))


def lib_api():
    from graph_odenet_amd import _lib
    return _lib.load(), _lib.check, _lib.stream_ptr


class Buf:
    """n floats (float64 with dtype) as a view into a NaN-filled device buffer PAD longer; mis: the view starts one float in."""

    def __init__(self, a, mis=False, dtype=torch.float32):
        if isinstance(a, int):
            n, a = a, None
        else:
            a = np.ascontiguousarray(a).reshape(-1)
            n = a.size
        self.n, self.off = n, (1 if mis else 0)
        self.full = torch.full((n + PAD,), NAN, dtype=dtype, device=dev())
        self.view = self.full[self.off:self.off + n]
        if a is not None and n:
            self.view.copy_(torch.from_numpy(a))
        assert (self.view.data_ptr() % 16 != 0) == bool(mis)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def result(self, written=None):
        """The view as numpy, after asserting that the first `written` elements hold no NaN and everything else still does."""
        w = self.n if written is None else written
        full = self.full.cpu()
        assert not torch.isnan(full[self.off:self.off + w]).any(), "an element was not written, or a NaN was read"
        assert torch.isnan(full[:self.off]).all() and torch.isnan(full[self.off + w:]).all(), "written outside its length"
        return full[self.off:self.off + self.n].numpy()


def lincomb_struct(coef, bufs):
    from graph_odenet_amd import _lib
    return _lib.lincomb([(float(c), b.view) for c, b in zip(coef, bufs)])


# ---- runners: the C ABI on a case's operands -------------------------------------------------------------------------------
def lincomb_operands(case, d):
    last = case.nterms - 1
    terms = [Buf(t, mis=("all" in case.mis or (j == last and "last" in case.mis))) for j, t in enumerate(d["terms"])]
    if case.inplace is None:
        out = Buf(case.n, mis=("all" in case.mis or "out" in case.mis))
    else:
        out = terms[0 if case.inplace == 0 else last]
    return out, terms, lincomb_struct(d["coef"], terms)


def run_lincomb(case, d):
    lib, check, stream = lib_api()
    out, terms, lc = lincomb_operands(case, d)
    check(lib.gode_lincomb_f32(out.ptr, ctypes.byref(lc), case.n, stream()), "gode_lincomb_f32")
    for t in terms:
        if t is not out:
            t.result()                                                  # the terms are read only
    return {"out": out.result()}


def err_operands(case, d):
    terms = [Buf(t, mis=(j == case.nterms - 1 and "term" in case.mis)) for j, t in enumerate(d["terms"])]
    return Buf(d["y0"], mis="y0" in case.mis), Buf(d["y1"], mis="y1" in case.mis), terms, lincomb_struct(d["coef"], terms)


def err_scratch(lib):
    return torch.empty(lib.gode_rk_errnorm_scratch_bytes(), dtype=torch.uint8, device=dev())


def run_err(case, d):
    lib, check, stream = lib_api()
    y0, y1, terms, lc = err_operands(case, d)
    out, scratch = Buf(1, mis=False, dtype=torch.float64), err_scratch(lib)
    sp = ctypes.c_void_p(scratch.data_ptr())
    if case.mode == 0:
        check(lib.gode_rk_errnorm_f32(out.ptr, y0.ptr, y1.ptr, ctypes.byref(lc), d["rtol"], d["atol"], case.n, sp, stream()), "gode_rk_errnorm_f32")
    else:
        check(lib.gode_rk_scaled_sumsq_f32(out.ptr, ctypes.byref(lc), y0.ptr, d["rtol"], d["atol"], case.n, sp, stream()), "gode_rk_scaled_sumsq_f32")
    return {"sum": float(out.result()[0])}


def run_lincomb_multi(case, d):
    from graph_odenet_amd import _lib
    lib, check, stream = lib_api()
    k = len(case.comps)
    ops = []
    for comp, cd in zip(case.comps, d["comps"]):
        if comp.n == 0:                                                 # not looked at: its output stays NaN
            ops.append((Buf(0), [], _lib.lincomb([])))
        else:
            ops.append(lincomb_operands(comp, cd))
    outs, lcs, ns = (ctypes.c_void_p * k)(), (_lib.LinComb * k)(), (ctypes.c_int64 * k)()
    for c, (out, _, lc) in enumerate(ops):
        outs[c], lcs[c], ns[c] = out.view.data_ptr(), lc, case.comps[c].n
    check(lib.gode_lincomb_multi_f32(outs, lcs, ns, k, stream()), "gode_lincomb_multi_f32")
    return {"comps": [{"out": out.result()} for out, _, _ in ops]}


def run_err_multi(case, d):
    from graph_odenet_amd import _lib
    lib, check, stream = lib_api()
    k = len(case.comps)
    ops = [err_operands(comp, cd) for comp, cd in zip(case.comps, d["comps"])]
    y0s, y1s, lcs, ns = (ctypes.c_void_p * k)(), (ctypes.c_void_p * k)(), (_lib.LinComb * k)(), (ctypes.c_int64 * k)()
    for c, (y0, y1, _, lc) in enumerate(ops):
        y0s[c], y1s[c], lcs[c], ns[c] = y0.view.data_ptr(), y1.view.data_ptr(), lc, case.comps[c].n
    out, scratch = Buf(k, dtype=torch.float64), err_scratch(lib)
    rtol, atol = d["comps"][0]["rtol"], d["comps"][0]["atol"]
    assert all((cd["rtol"], cd["atol"]) == (rtol, atol) for cd in d["comps"])
    check(lib.gode_rk_errnorm_multi_f32(out.ptr, y0s, y1s, lcs, ns, k, rtol, atol, ctypes.c_void_p(scratch.data_ptr()), stream()),
          "gode_rk_errnorm_multi_f32")
    return {"comps": [{"sum": float(v)} for v in out.result()]}


def out_operand(n, acc, out0, mis=False):
    return Buf(out0, mis=mis) if acc else Buf(n, mis=mis)


def run_parts(case, d):
    lib, check, stream = lib_api()
    part, out = Buf(d["part"]), out_operand(case.len, case.acc, d["out0"], case.mis_out)
    check(lib.gode_reduce_parts_f32(out.ptr, part.ptr, case.n_part, case.len, case.scale, case.acc, stream()), "gode_reduce_parts_f32")
    part.result()
    return {"out": out.result()}


def run_parts2(case, d):
    lib, check, stream = lib_api()
    pa, pb = Buf(d["part"]), Buf(d["part_b"])
    oa, ob = out_operand(case.len, case.acc, d["out0"]), out_operand(case.len, case.acc, d["out0_b"])
    check(lib.gode_reduce_parts2_f32(oa.ptr, pa.ptr, ob.ptr, pb.ptr, case.n_part, case.len, case.scale, case.acc, stream()),
          "gode_reduce_parts2_f32")
    return {"out_a": oa.result(), "out_b": ob.result()}


def run_segs(case, d):
    from graph_odenet_amd import _lib
    lib, check, stream = lib_api()
    arr = (_lib.ReduceSeg * len(case.segs))()
    keep, outs = [], []
    for k, (s, sd) in enumerate(zip(case.segs, d["segs"])):
        part, out = Buf(sd["part"]), Buf(s["len"] + D.SEG_SURPLUS)
        w = Buf(sd["w"]) if s["wrow"] else None
        keep += [part, w]
        outs.append(out)
        q = arr[k]
        q.out, q.part = out.view.data_ptr(), (part.view.data_ptr() if s["n_part"] else None)
        q.n_part, q.ld, q.col0, q.col_stride, q.len = s["n_part"], s["ld"], s["col0"], s["cs"], s["len"]
        q.w_row0, q.time_len = (w.view.data_ptr() if w is not None else None), s["time_len"]
    at = None if case.at_null else Buf(1)
    check(lib.gode_reduce_segments_f32(arr, len(case.segs), d["t"], at.ptr if at is not None else None, stream()), "gode_reduce_segments_f32")
    res = {"out%d" % k: out.result(written=s["len"])[:s["len"]] for k, (s, out) in enumerate(zip(case.segs, outs))}
    if at is not None:
        res["at"] = float(at.result()[0])
    return res


def run_colsum(case, d):
    lib, check, stream = lib_api()
    n_rows, dd = case.n_rows, case.d
    X, out = Buf(d["X"], mis=case.mis_x), out_operand(dd, case.acc, d["out0"])
    floats = lib.gode_colsum_scratch_bytes(n_rows, dd) // 4
    assert floats == D.colsum_blocks(n_rows) * dd
    xp = X.ptr if n_rows else None
    scratch = Buf(floats)
    check(lib.gode_colsum_f32(out.ptr, xp, n_rows, dd, case.scale, case.acc, scratch.ptr, stream()), "gode_colsum_f32")
    scratch = Buf(floats)                                               # the first half alone, into a fresh scratch
    n_parts = ctypes.c_int64(-1)
    check(lib.gode_colsum_parts_f32(xp, n_rows, dd, scratch.ptr, ctypes.byref(n_parts), stream()), "gode_colsum_parts_f32")
    assert n_parts.value == D.colsum_blocks(n_rows)
    X.result()
    return {"out": out.result(), "parts": scratch.result(written=n_parts.value * dd).reshape(n_parts.value, dd)}


RUNNERS = {"lincomb": run_lincomb, "err": run_err, "lincomb_multi": run_lincomb_multi, "err_multi": run_err_multi, "parts": run_parts,
           "parts2": run_parts2, "segs": run_segs, "colsum": run_colsum}


def same_bits(a, b):
    if isinstance(a, float):
        return a == b
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def compare(name, kind, got, ref):
    """got against {quantity: (float64 reference, bound)}: equal on the exact data, inside the bound on the real data."""
    assert set(got) == set(ref), (name, sorted(got), sorted(ref))
    if kind == "exact":
        bad = [k for k in ref if not D.exact_equal(got[k], ref[k][0])]
        print("%s exact: %s" % (name, "equal" if not bad else "UNEQUAL " + ", ".join(bad)))
        assert not bad, "%s: not the float64 result on the exact data: %s" % (name, ", ".join(
            "%s (err %.3e)" % (k, D.error_figures(got[k], ref[k][0], np.inf)[0]) for k in bad))
    else:
        figs = {k: D.error_figures(got[k], *ref[k]) for k in ref}
        ERRORS[name] = figs
        print("%s real: %s" % (name, "  ".join("%s=%.2e (%.3f of bound)" % (k, m, fr) for k, (m, fr) in figs.items())))
        bad = [k for k in ref if not D.within(got[k], *ref[k])]
        assert not bad, "%s: outside the derived bound: %s" % (name, ", ".join("%s (%.3f of it)" % (k, figs[k][1]) for k in bad))


def run_case(case):
    run = RUNNERS[case.family]
    multi = hasattr(case, "comps")
    for kind in ("exact", "real"):
        d, ref = D.inputs(case, kind), D.reference(case, kind)
        got = run(case, d)
        again = run(case, d)                                            # fixed summation order: bit-identical
        if not multi:
            compare(case.id, kind, got, ref)
            for k in got:
                assert same_bits(got[k], again[k]), k + " differs between two runs"
            continue
        assert len(got["comps"]) == len(case.comps)
        for c, comp in enumerate(case.comps):
            g, a = got["comps"][c], again["comps"][c]
            key = "out" if case.family == "lincomb_multi" else "sum"
            assert same_bits(g[key], a[key]), "component %d differs between two runs" % c
            if comp.n == 0:
                assert g["out"].size == 0
                continue
            compare("%s[%d]" % (case.id, c), kind, g, ref["comps"][c])
            single = RUNNERS[comp.family](comp, d["comps"][c])
            assert same_bits(g[key], single[key]), "component %d of the multi form is not the single form's bit for bit" % c


@pytest.mark.parametrize("case", D.LINCOMB_CASES, ids=ID)
def test_lincomb_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.LINCOMB_MULTI_CASES, ids=ID)
def test_lincomb_multi_vs_float64_and_the_single_form(case):
    run_case(case)


@pytest.mark.parametrize("case", D.ERR_CASES, ids=ID)
def test_error_sums_vs_float64(case):
    """gode_rk_errnorm_f32 (cases _m0) and gode_rk_scaled_sumsq_f32 (_m1).  The build has no fast-math flag, so the float32
    division is correctly rounded and the exact sums are compared with ==."""
    run_case(case)


@pytest.mark.parametrize("case", D.ERR_MULTI_CASES, ids=ID)
def test_errnorm_multi_vs_float64_and_the_single_form(case):
    run_case(case)


@pytest.mark.parametrize("case", D.PARTS_CASES, ids=ID)
def test_reduce_parts_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.PARTS2_CASES, ids=ID)
def test_reduce_parts2_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.SEGS_CASES, ids=ID)
def test_reduce_segments_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.COLSUM_CASES, ids=ID)
def test_colsum_and_colsum_parts_vs_float64(case):
    run_case(case)


# ---- through the ops wrappers ----------------------------------------------------------------------------------------------
def to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("kind", ("exact", "real"))
def test_ops_wrappers(kind):
    """lincomb_, lincomb_multi_, rk_error_sumsq, rk_scaled_sumsq, reduce_parts_, reduce_parts2_, reduce_segments_, colsum_ and
    colsum_parts on two or three of the cases each, to the same comparisons."""
    from graph_odenet_amd import ops
    B = D.BY_ID
    for name in ("lincomb/n1028", "lincomb/n1023", "lincomb/terms8_n1028"):
        case, d = B[name], D.inputs(B[name], kind)
        out = torch.full((case.n,), NAN, device=dev())
        ops.lincomb_(out, [(float(c), to(t)) for c, t in zip(d["coef"], d["terms"])])
        compare("ops." + name, kind, {"out": host(out)}, D.reference(case, kind))
    case = B["lincomb_multi/count3"]
    d, ref = D.inputs(case, kind), D.reference(case, kind)
    terms = [[(float(c), to(t)) for c, t in zip(cd["coef"], cd["terms"])] for cd in d["comps"]]
    outs = [tl[0][1] if comp.inplace == 0 else torch.full((comp.n,), NAN, device=dev()) for comp, tl in zip(case.comps, terms)]
    ops.lincomb_multi_(outs, terms)
    for c, out in enumerate(outs):
        compare("ops.%s[%d]" % (case.id, c), kind, {"out": host(out)}, ref["comps"][c])
    for name in ("err/n1028_m0", "err/n1025_m0", "err/terms8_n1028_m0", "err/n1028_m1", "err/n1025_m1", "err/terms8_n1025_m1"):
        case, d = B[name], D.inputs(B[name], kind)
        terms = [(float(c), to(t)) for c, t in zip(d["coef"], d["terms"])]
        if case.mode == 0:
            out = ops.rk_error_sumsq(to(d["y0"]), to(d["y1"]), terms, d["rtol"], d["atol"])
        else:
            out = ops.rk_scaled_sumsq(terms, to(d["y0"]), d["rtol"], d["atol"])
        assert out.dtype == torch.float64 and out.numel() == 1
        compare("ops." + name, kind, {"sum": float(out.item())}, D.reference(case, kind))
    for name in ("parts/37x1000_acc0_scale1", "parts/25x33_acc1_scale-0.5", "parts/64x4096_acc1_scale-0.5"):
        case, d = B[name], D.inputs(B[name], kind)
        out = to(d["out0"]) if case.acc else torch.full((case.len,), NAN, device=dev())
        ops.reduce_parts_(out, to(d["part"]), scale=case.scale, accumulate=bool(case.acc))
        compare("ops." + name, kind, {"out": host(out)}, D.reference(case, kind))
    for case in D.PARTS2_CASES:                                         # the wrapper overwrites with scale 1
        d = D.inputs(case, kind)
        oa, ob = torch.full((case.len,), NAN, device=dev()), torch.full((case.len,), NAN, device=dev())
        ops.reduce_parts2_(oa, to(d["part"]), ob, to(d["part_b"]))
        compare("ops." + case.id, kind, {"out_a": host(oa), "out_b": host(ob)},
                {"out_a": D.sum_ref(d["part"], 1.0, 0, None), "out_b": D.sum_ref(d["part_b"], 1.0, 0, None)})
    for shape in ((256, 128), (257, 301), (65, 2667)):                  # colsum4 / colsum_kernel / colsum_wide_kernel
        case = next(c for c in D.COLSUM_CASES if (c.n_rows, c.d) == shape)
        name, d = case.id, D.inputs(case, kind)
        X, ref = to(d["X"]), D.reference(case, kind)
        out = to(d["out0"]) if case.acc else torch.full((case.d,), NAN, device=dev())
        ops.colsum_(out, X, scale=case.scale, accumulate=bool(case.acc))
        scratch = torch.empty(D.colsum_blocks(case.n_rows) * case.d * 4, dtype=torch.uint8, device=dev())
        n_parts = ops.colsum_parts(X, scratch)
        assert n_parts == D.colsum_blocks(case.n_rows)
        compare("ops." + name, kind, {"out": host(out), "parts": host(scratch.view(torch.float32)).reshape(n_parts, case.d)}, ref)
    for name in ("segs/eight", "segs/time_two"):
        case, d = B[name], D.inputs(B[name], kind)
        outs = [torch.full((s["len"],), NAN, device=dev()) for s in case.segs]
        at = None if case.at_null else torch.full((1,), NAN, device=dev())
        segs = [(out, (to(sd["part"]) if s["n_part"] else 0), s["n_part"], s["ld"], s["col0"], s["cs"], s["len"],
                 (to(sd["w"]) if s["wrow"] else None), s["time_len"]) for s, sd, out in zip(case.segs, d["segs"], outs)]
        ops.reduce_segments_(segs, t=d["t"], at=at)
        got = {"out%d" % k: host(out) for k, out in enumerate(outs)}
        if at is not None:
            got["at"] = float(at.item())
        compare("ops." + name, kind, got, D.reference(case, kind))
