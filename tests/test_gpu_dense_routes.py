"""Every route of the fp32 GroupNorm-time-GEMM kernels (csrc/gemm.hip) against float64: gode_gn_time_gemm_f32 / _xout_f32 /
_xout_aux_f32 / _pair_f32, gode_gn_time_gemm_bwd_f32, gode_wgrad_f32, gode_group_norm_f32_fwd / _bwd.

The cases, the limits they bracket, the float64 reference and the derived bounds are in tests/dense_routes_design.py;
test_dense_routes.py checks on the CPU that every case reaches its routes, that the exact data is exact, that plain float32
in four summation orders stays inside the bounds on the real data, that no bound is looser than the bar of the older tests in
test_gpu_kernels.py, the host-side answers of the entry points, and that fifteen planted defects are each rejected by the
comparisons used here.

Every case drives the C ABI itself.  Every operand is a view into a NaN-filled buffer eight floats longer than it (a
misaligned operand starts one float into its buffer); every output - S, x_out, aux_out, dx, the dgamma / dbeta partials, the
weight-gradient partials - is NaN before the call, no NaN may remain inside the written length and every float outside it is
NaN afterwards.  ALL gode_gemm_bwd_parts(n) rows of the dgamma / dbeta buffers are summed (in float64), the rows no block owns
included.  CG = 0 cases run on the exact data (np.array_equal against float64; the weight-gradient partials summed in float64
and compared with ==), the others on the real data (elementwise inside the derived bound).  Every case stays below 65 536
rows and the options are asserted to be at their defaults on entry, so neither the producer / consumer kernels of gemm_pc.hip
nor wgrad_split_kernel is ever selected; the one option changed (inside try / finally) is gemm_split = 1 for the split-bf16
forward cases.

Routes and the cases that reach them (family/case; test_dense_routes.py recomputes them):
  gn_gemm_fwd_kernel<NJ, CG>, all 16              fwd/sweep_d{16,32,64,128}_cg{0,1,2,4} (n = 37: two tiles and a ragged one)
  ... <8, CG, AUX>, all 4; 1 .. 8 terms           fwd/aux_cg{0,1,2,4}, aux_terms{2..7}, aux_trip2
  gn_gemm_fwd_split_kernel<CG, NX>, all 12        fwd/split_cg{0,1,2,4}_terms{1,2,3|5}, split_trip2
  gn_narrow_{fwd,bwd}_kernel / narrow_wgrad, 16   fwd/narrow_*, bwd/narrow_*, wgrad/narrow_*
  gn_gemm_bwd_kernel / wgrad_kernel, all 16       bwd/sweep_*, wgrad/sweep_*
  grid.y = 2 for all 16, and the two-call form    pair/sweep_*, pair/two_calls_d24, two_calls_mis_x0
  tile edges n = 1, 15, 16, 17, 63, 64, 65        fwd/edge_n*, narrow_edge_n* (with x_out), bwd/edge_n*, narrow_edge_n* (with pre):
                                                  four channels per group, where a misplaced row or term shows
  1 .. 8 terms where the result depends on x      */trip2_d16_terms*, */narrow_terms*, */generic_terms* (CG 0, 4 or 5), fwd/aux_*
  weight gradient n = 0, 31, 32, 33               wgrad/edge_n*, narrow_edge_n*, generic_edge_n*
  second trip of the grid-stride loops            */trip2_d16_terms{1..8} (n = 32 789; weight gradient 16 417), trip2_d{32,64,128},
                                                  wgrad/trip2_d{32,64,128}_exact (the reduction over rows bit for bit),
                                                  narrow_trip2, generic_trip2, aux_trip2, split_trip2, pair/trip2, gn/trip2
  generic kernels: d = 24/24, 40/8, 96/32, CG 8, 16, d_in != d_out, d_in = 2 048 (> 64 KB of LDS in the VJP), a misaligned
  first term / S / dS / dx                        */generic_*, */mis_*
  stand-alone GroupNorm                           gn/*

Bit-for-bit cross-checks: the second-trip rows of a 32 789-row forward launch (loaded through the prefetch chain) against a
launch over those rows alone (the first-tile chain), 1 .. 8 terms at d = 16 and 128 and once at d = 32 and 64, S, x_out and
the AUX output; the pair launch against two single calls; the AUX launch's S against the plain launch's; stand-alone GroupNorm against the generic GEMM kernels under an
identity W.  groups = 0 with partial buffers leaves them untouched on every route (include/graphode.h says so).  A call that
returns an error before launching writes nothing.

Measured on an MI355X (real data, worst case of each quantity: the suite's metric max |got - ref| / max(1, max |ref|), and the
largest fraction of the derived bound any element used; profiles/dense_routes_errors.txt has every case; all 52 exact
comparisons held bit for bit, and so did every cross-check - no defect was found in gemm.hip or dense_common.h):
  x_out / aux_out   1.9e-7 (fwd/aux_trip2); 0.68 of the bound (fwd/generic_trip2) / 0.63 (fwd/aux_trip2)
  S / Sb            1.5e-5 at one channel per group (pair/two_calls_d24); 0.37 of the bound (fwd/generic_16x34)
  stand-alone y     6.1e-5 at one channel per group, 0.47 of the bound (gn/d24_g24)
  dx                3.1e-5 at one channel per group (gn/d24_g24); 0.64 of the bound (bwd/narrow_d64_cg4, 6.2e-8)
  dgamma / dbeta    2.9e-7 / 2.7e-7 (bwd/trip2_d128); 0.10 / 0.04 of the bound (bwd/narrow_edge_n1 / gn/d24_g24)
  dW / its time row 5.1e-5 at one channel per group (wgrad/sweep_d32_cg1); 0.22 / 0.08 of the bound (wgrad/sweep_d128_cg1 /
                    wgrad/generic_terms7); the second trip of the weight gradient also compares == on wgrad/trip2_d*_exact

DENSE_ROUTES_ERRORS=<file>: the figures of the run are written there (profiles/dense_routes_errors.txt is such a file).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_routes_design as D                                         # noqa: E402

pytestmark = pytest.mark.gpu
ERRORS, EXACT_OK = {}, []
NAN = float("nan")
PAD = 8
ID = lambda c: c.name                                                   # noqa: E731
DEFAULTS = {"gemm_split": 2, "wgrad_split": 8, "wgrad_split_small": 0, "bwd_pc": 1, "fwd_pc": 3, "bwd_wgrad": 1}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def lib_api():
    from graph_odenet_amd import _lib
    return _lib.load(), _lib.check, _lib.stream_ptr


@pytest.fixture(scope="module", autouse=True)
def defaults_and_errors_file():
    lib = lib_api()[0]
    for name, value in DEFAULTS.items():
        assert lib.gode_get_option(name.encode()) == value, "option %s is not at its default" % name
    yield
    for name, value in DEFAULTS.items():
        assert lib.gode_get_option(name.encode()) == value, "option %s was left changed" % name
    path = os.environ.get("DENSE_ROUTES_ERRORS")
    if path and ERRORS:
        with open(path, "w") as f:
            f.write("# real data, every case and quantity against float64: max |got - ref| / max(1, max |ref|), and the largest\n")
            f.write("# fraction of the derived bound (tests/dense_routes_design.py) any element used\n")
            for name, figs in ERRORS.items():
                f.write("%-34s %s\n" % (name, "  ".join("%s=%.2e (%.3f of bound)" % (k, m, fr) for k, (m, fr) in figs.items())))
            f.write("# exact data (CG = 0): equal to float64 bit for bit\n")
            for name in EXACT_OK:
                f.write("%-34s equal\n" % name)


class Buf:
    """A float32 array as a view into a NaN-filled device buffer PAD longer; mis: the view starts one float (4 bytes) in."""

    def __init__(self, a, mis=False):
        if isinstance(a, (int, np.integer)):
            n, a, self.shape = int(a), None, (int(a),)
        else:
            self.shape = a.shape
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            n = a.size
        self.n, self.off = n, (1 if mis else 0)
        self.full = torch.full((n + PAD,), NAN, dtype=torch.float32, device=dev())
        self.view = self.full[self.off:self.off + n]
        if a is not None and n:
            self.view.copy_(torch.from_numpy(a))
        self.addr = self.full.data_ptr() + 4 * self.off
        assert (self.addr % 16 != 0) == bool(mis)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def result(self, written=None):
        """The view as numpy, after asserting that the first `written` elements hold no NaN and everything else still does."""
        w = self.n if written is None else written
        full = self.full.cpu()
        assert not torch.isnan(full[self.off:self.off + w]).any(), "an element was not written, or a NaN was read"
        assert torch.isnan(full[:self.off]).all() and torch.isnan(full[self.off + w:]).all(), "written outside its length"
        return full[self.off:self.off + self.n].numpy().reshape(self.shape)

    def untouched(self):
        return bool(torch.isnan(self.full).all().item())


def opt(a):
    return None if a is None else a.ptr


def lincomb_struct(coef, bufs):
    from graph_odenet_amd import _lib
    lc = _lib.LinComb()
    lc.n = len(bufs)
    for j, (c, b) in enumerate(zip(coef, bufs)):
        lc.coef[j], lc.ptr[j] = float(c), b.addr
    return lc


class Operands:
    """The device operands every family shares: the terms, gamma, beta."""

    def __init__(self, case, d):
        self.terms = [Buf(t, mis=(j == 0 and case.mis == "x0")) for j, t in enumerate(d["terms"])]
        self.lc = lincomb_struct(d["coef"], self.terms)
        self.gamma = None if d["gamma"] is None else Buf(d["gamma"])
        self.beta = None if d["beta"] is None else Buf(d["beta"])

    def read_only(self):
        for b in self.terms + [self.gamma, self.beta]:
            if b is not None:
                b.result()


# ---- runners: the C ABI on a case's operands -------------------------------------------------------------------------------
def run_fwd(case, d, aux=None, rows=None):
    """rows = (a, b): the launch over rows a .. b - 1 alone."""
    lib, check, stream = lib_api()
    if rows is not None:
        d = dict(d, terms=[t[rows[0]:rows[1]] for t in d["terms"]])
    n = d["terms"][0].shape[0]
    ops, W = Operands(case, d), Buf(d["W"])
    S = Buf(np.full((n, case.d_out), NAN, np.float32), mis=case.mis == "S")
    xout = Buf(np.full((n, case.d_in), NAN, np.float32)) if case.xout else None
    with_aux = case.aux if aux is None else aux
    auxo = Buf(np.full((n, case.d_in), NAN, np.float32)) if with_aux else None
    ac = (ctypes.c_float * len(d["aux_coef"]))(*[float(c) for c in d["aux_coef"]]) if with_aux else None
    if case.split:
        check(lib.gode_set_option(b"gemm_split", 1), "gemm_split")
    try:
        check(lib.gode_gn_time_gemm_xout_aux_f32(ctypes.byref(ops.lc), n, case.d_in, case.groups, d["eps"], opt(ops.gamma), opt(ops.beta), W.ptr,
                                                 case.d_out, case.has_time, d["t"], S.ptr, opt(xout), ac, opt(auxo), stream()),
              "gode_gn_time_gemm_xout_aux_f32")
    finally:
        if case.split:
            check(lib.gode_set_option(b"gemm_split", DEFAULTS["gemm_split"]), "gemm_split")
    ops.read_only(); W.result()
    res = {"S": S.result()}
    if xout is not None:
        res["xout"] = xout.result()
    if auxo is not None:
        res["aux"] = auxo.result()
    return res


def run_pair(case, d):
    lib, check, stream = lib_api()
    n = case.n
    ops, Wa, Wb = Operands(case, d), Buf(d["W"]), Buf(d["Wb"])
    Sa, Sb = Buf(np.full((n, case.d_in), NAN, np.float32)), Buf(np.full((n, case.d_in), NAN, np.float32))
    xout = Buf(np.full((n, case.d_in), NAN, np.float32)) if case.xout else None
    check(lib.gode_gn_time_gemm_pair_f32(ctypes.byref(ops.lc), n, case.d_in, case.groups, d["eps"], opt(ops.gamma), opt(ops.beta), Wa.ptr, Wb.ptr,
                                         case.has_time, d["t"], Sa.ptr, Sb.ptr, opt(xout), stream()), "gode_gn_time_gemm_pair_f32")
    ops.read_only()
    res = {"S": Sa.result(), "Sb": Sb.result()}
    if xout is not None:
        res["xout"] = xout.result()
    return res


def run_bwd(case, d, raw=False):
    lib, check, stream = lib_api()
    n, n_part = case.n, lib.gode_gemm_bwd_parts(case.n)
    assert n_part == D.bwd_parts(n)
    ops, W, dS = Operands(case, d), Buf(d["W"]), Buf(d["dS"], mis=case.mis == "dS")
    dx = Buf(np.full((n, case.d_in), NAN, np.float32), mis=case.mis == "dx")
    dg, db = Buf(np.full((n_part, case.d_in), NAN, np.float32)), Buf(np.full((n_part, case.d_in), NAN, np.float32))
    pre = [Buf(p) for p in d["pre"]]
    plc = lincomb_struct(d["pre_coef"], pre) if pre else None
    check(lib.gode_gn_time_gemm_bwd_f32(ctypes.byref(ops.lc), n, case.d_in, case.groups, d["eps"], opt(ops.gamma), W.ptr, case.d_out, case.has_time,
                                        dS.ptr, d["out_scale"], ctypes.byref(plc) if plc is not None else None, dx.ptr, dg.ptr, db.ptr, stream()),
          "gode_gn_time_gemm_bwd_f32")
    ops.read_only(); W.result(); dS.result()
    for p in pre:
        p.result()
    res = {"dx": dx.result()}
    if case.groups:
        g, b = dg.result(), db.result()                                 # every one of the n_part rows is written
        res.update(dgamma=g.astype(np.float64).sum(0), dbeta=b.astype(np.float64).sum(0))
        if raw:
            res.update(dgamma_parts=g, dbeta_parts=b)
    else:
        assert dg.untouched() and db.untouched(), "groups = 0: the partial buffers are left alone"
    return res


def run_wgrad(case, d):
    lib, check, stream = lib_api()
    n, n_part, K = case.n, lib.gode_wgrad_parts(case.n), case.d_in + case.has_time
    assert n_part == D.wgrad_blocks(n)
    ops, dS = Operands(case, d), Buf(d["dS"], mis=case.mis == "dS")
    part = Buf(np.full((n_part, K, case.d_out), NAN, np.float32))
    check(lib.gode_wgrad_f32(ctypes.byref(ops.lc), n, case.d_in, case.groups, d["eps"], opt(ops.gamma), opt(ops.beta), dS.ptr if n else None,
                             case.d_out, case.has_time, part.ptr, stream()), "gode_wgrad_f32")
    ops.read_only()
    p = part.result()
    if n == 0:
        assert n_part == 1 and not p.any(), "no rows: one all-zero partial"
    total = p.astype(np.float64).sum(0)
    res = {"dW": total[case.has_time:]}
    if case.has_time:
        res["dW0"] = total[0]
    return res


def run_gn(case, d, raw=False):
    lib, check, stream = lib_api()
    n, n_part = case.n, lib.gode_group_norm_parts(case.n)
    assert n_part == D.gen_blocks(n)
    x, dy = Buf(d["terms"][0]), Buf(d["dS"])
    gamma = None if d["gamma"] is None else Buf(d["gamma"])
    beta = None if d["beta"] is None else Buf(d["beta"])
    y, dx = Buf(np.full((n, case.d_in), NAN, np.float32)), Buf(np.full((n, case.d_in), NAN, np.float32))
    dg, db = Buf(np.full((n_part, case.d_in), NAN, np.float32)), Buf(np.full((n_part, case.d_in), NAN, np.float32))
    check(lib.gode_group_norm_f32_fwd(x.ptr, n, case.d_in, case.groups, d["eps"], opt(gamma), opt(beta), y.ptr, stream()), "gode_group_norm_f32_fwd")
    check(lib.gode_group_norm_f32_bwd(x.ptr, n, case.d_in, case.groups, d["eps"], opt(gamma), dy.ptr, dx.ptr, dg.ptr, db.ptr, stream()),
          "gode_group_norm_f32_bwd")
    x.result(); dy.result()
    g, b = dg.result(), db.result()
    res = {"y": y.result(), "dx": dx.result(), "dgamma": g.astype(np.float64).sum(0), "dbeta": b.astype(np.float64).sum(0)}
    if raw:
        res.update(dgamma_parts=g, dbeta_parts=b)
    return res


RUNNERS = {"fwd": run_fwd, "pair": run_pair, "bwd": run_bwd, "wgrad": run_wgrad, "gn": run_gn}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                                                        b.view(np.int32 if b.dtype == np.float32 else np.int64))


def compare(name, kind, got, ref):
    """got against {quantity: (float64 reference, bound)}: equal on the exact data, inside the bound on the real data."""
    assert set(got) == set(ref), (name, sorted(got), sorted(ref))
    if kind == "exact":
        bad = [k for k in ref if not D.exact_equal(got[k], ref[k][0])]
        print("%s exact: %s" % (name, "equal" if not bad else "UNEQUAL " + ", ".join(bad)))
        assert not bad, "%s: not the float64 result on the exact data: %s" % (name, ", ".join(
            "%s (err %.3e)" % (k, D.error_figures(got[k], ref[k][0], np.inf)[0]) for k in bad))
        EXACT_OK.append(name)
    else:
        figs = {k: D.error_figures(got[k], *ref[k]) for k in ref}
        ERRORS[name] = figs
        print("%s real: %s" % (name, "  ".join("%s=%.2e (%.3f of bound)" % (k, m, fr) for k, (m, fr) in figs.items())))
        bad = [k for k in ref if not D.within(got[k], *ref[k])]
        assert not bad, "%s: outside the derived bound: %s" % (name, ", ".join("%s (%.3f of it)" % (k, figs[k][1]) for k in bad))
        assert all(fr <= 1.0 for _, fr in figs.values())


def run_case(case):
    kind = case.kinds[0]
    d = D.inputs(case, kind)
    got = RUNNERS[case.family](case, d)
    compare(case.id, kind, got, D.reference(case, kind))
    return d, got


@pytest.mark.parametrize("case", D.FWD_CASES, ids=ID)
def test_forward_vs_float64(case):
    """gode_gn_time_gemm_xout_aux_f32 (what _f32 and _xout_f32 forward to).  An AUX launch's S and x_out are the plain launch's
    bit for bit."""
    d, got = run_case(case)
    if case.aux:
        plain = run_fwd(case, d, aux=False)
        assert same_bits(plain["S"], got["S"]), "S of the AUX launch is not the plain launch's"
        if case.xout:
            assert same_bits(plain["xout"], got["xout"])


@pytest.mark.parametrize("case", D.PAIR_CASES, ids=ID)
def test_pair_vs_float64_and_two_single_calls(case):
    d, got = run_case(case)
    a = run_fwd(case, d)
    b = run_fwd(D.Case("fwd", "pair_b", (), **{k: v for k, v in case.__dict__.items() if k not in ("family", "name", "reaches", "xout")}), dict(d, W=d["Wb"]))
    assert same_bits(a["S"], got["S"]) and same_bits(b["S"], got["Sb"]), "the pair launch is not the two single calls bit for bit"
    if case.xout:
        assert same_bits(a["xout"], got["xout"])


@pytest.mark.parametrize("case", D.BWD_CASES, ids=ID)
def test_vjp_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.WGRAD_CASES, ids=ID)
def test_weight_gradient_vs_float64(case):
    run_case(case)


@pytest.mark.parametrize("case", D.GN_CASES, ids=ID)
def test_group_norm_vs_float64(case):
    run_case(case)


# ---- bit-for-bit cross-checks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nterms", range(1, 9))
def test_prefetched_rows_are_the_first_tile_chains(nterms):
    """The second-trip rows of a 32 789-row forward launch are combined by issue_terms2 / fold_terms2 between the halves of the
    MFMA panel; a launch over those rows alone combines them by load_tile_n (AUX: by the first tile's pairwise chain).  Same
    bits: S, x_out and the AUX output, at d = 16 and (AUX) d = 128."""
    case = D.BY_ID["fwd/trip2_d16_terms%d" % nterms]
    first = D.first_trip_rows("fwd", case)
    assert case.n - first == 21
    xo = D.Case("fwd", "prefetch_d16", (), **{k: v for k, v in case.__dict__.items() if k not in ("family", "name", "reaches", "xout")}, xout=True)
    d = D.inputs(case, case.kinds[0])
    whole, tail = run_fwd(xo, d), run_fwd(xo, d, rows=(first, case.n))
    for k in ("S", "xout"):
        assert same_bits(whole[k][first:], tail[k]), "%s of the prefetched rows differs from the first-tile chain's" % k
    aux = D.Case("fwd", "prefetch_aux", (), d_in=128, d_out=128, groups=32, n=case.n, nterms=nterms, aux=True, xout=True)
    rng = np.random.RandomState(nterms)
    da = {"terms": [rng.standard_normal((case.n, 128)).astype(np.float32) for _ in range(nterms)], "coef": np.array(D.REAL_COEF[:nterms], np.float32),
          "aux_coef": np.array(D.REAL_AUX_COEF[:nterms], np.float32), "gamma": (rng.rand(128) + 0.5).astype(np.float32),
          "beta": (rng.rand(128) - 0.5).astype(np.float32), "W": (rng.standard_normal((129, 128)) / 11.3).astype(np.float32), "t": D.REAL_T, "eps": D.EPS}
    whole, tail = run_fwd(aux, da), run_fwd(aux, da, rows=(first, case.n))
    for k in ("S", "xout", "aux"):
        assert same_bits(whole[k][first:], tail[k]), "AUX launch: %s of the prefetched rows differs from the first-tile chain's" % k


@pytest.mark.parametrize("name", ["trip2_d32", "trip2_d64", "trip2_d128"])
def test_prefetched_rows_are_the_first_tile_chains_at_every_width(name):
    """The same promise once per NJ above d = 16: S and x_out of the second-trip rows against a launch over those rows alone."""
    case = D.BY_ID["fwd/" + name]
    first = D.first_trip_rows("fwd", case)
    xo = D.Case("fwd", "prefetch_" + name, (), **{k: v for k, v in case.__dict__.items() if k not in ("family", "name", "reaches", "xout")}, xout=True)
    d = D.inputs(case, case.kinds[0])
    whole, tail = run_fwd(xo, d), run_fwd(xo, d, rows=(first, case.n))
    for k in ("S", "xout"):
        assert same_bits(whole[k][first:], tail[k]), "%s of the prefetched rows differs from the first-tile chain's" % k


@pytest.mark.parametrize("shape", [(24, 24), (40, 8), (96, 32)])
def test_group_norm_is_the_generic_gemm_under_identity(shape):
    """Stand-alone GroupNorm forward and backward against the generic GEMM kernels with W = I and no time row: the products add
    exact zeros, so y, dx and every partial row are the same bits."""
    dd, groups = shape
    gn = D.Case("gn", "identity_d%d" % dd, (), d_in=dd, d_out=dd, groups=groups, n=D.SWEEP_N, nterms=1, has_time=0)
    d = D.inputs(gn, "real")
    alone = run_gn(gn, d, raw=True)
    kw = dict(d_in=dd, d_out=dd, groups=groups, n=D.SWEEP_N, nterms=1, has_time=0)
    dg = dict(d, W=np.eye(dd, dtype=np.float32), out_scale=1.0, pre=[], pre_coef=np.zeros(0, np.float32))
    fwd = run_fwd(D.Case("fwd", "identity", (), **kw), dg)
    bwd = run_bwd(D.Case("bwd", "identity", (), **kw), dg, raw=True)
    assert same_bits(fwd["S"], alone["y"]) and same_bits(bwd["dx"], alone["dx"])
    assert same_bits(bwd["dgamma_parts"], alone["dgamma_parts"]) and same_bits(bwd["dbeta_parts"], alone["dbeta_parts"])


# ---- what is not written ----------------------------------------------------------------------------------------------------
def test_groups_0_leaves_the_partial_buffers_untouched():
    """include/graphode.h: without GroupNorm dgamma_part and dbeta_part are left untouched - on the MFMA kernel, the narrow
    kernel and the generic kernel alike (run_bwd asserts it on every CG = 0 case; here one of each by name)."""
    for name in ("bwd/sweep_d32_cg0", "bwd/narrow_d64_cg0", "bwd/generic_24x7", "bwd/mis_dS", "bwd/sweep_d128_cg0"):
        case = D.BY_ID[name]
        assert case.groups == 0
        run_bwd(case, D.inputs(case, "exact"))


def test_error_returns_write_nothing():
    """Every refusal comes before the launch: S, x_out, aux_out, dx and the partial buffers are still all NaN."""
    lib, _, stream = lib_api()
    n, d = 8, 128
    x, W, gam, bet = Buf(np.ones((n, d), np.float32)), Buf(np.ones((d + 1, d), np.float32)), Buf(np.ones(d, np.float32)), Buf(np.zeros(d, np.float32))
    lc = lincomb_struct([1.0], [x])
    ac = (ctypes.c_float * 1)(1.0)
    outs = {k: Buf(np.full((n, d), NAN, np.float32)) for k in ("S", "xout", "aux", "dx", "dg", "db")}
    mis = Buf(np.full((n, d), NAN, np.float32), mis=True)

    def fwd(dd=d, groups=32, S=outs["S"], xout=None, aux=None, n_rows=n):
        return lib.gode_gn_time_gemm_xout_aux_f32(ctypes.byref(lc), n_rows, dd, groups, 1e-5, gam.ptr, bet.ptr, W.ptr, dd, 1, 0.5, S.ptr, opt(xout),
                                                  ac if aux is not None else None, opt(aux), stream())

    def bwd(dd=d, groups=32, dg=outs["dg"], db=outs["db"], n_rows=n):
        return lib.gode_gn_time_gemm_bwd_f32(ctypes.byref(lc), n_rows, dd, groups, 1e-5, gam.ptr, W.ptr, dd, 1, x.ptr, 1.0, None, outs["dx"].ptr,
                                             opt(dg), opt(db), stream())
    assert fwd(dd=64, aux=outs["aux"]) == D.E_UNSUPPORTED                                  # aux_out off d = 128
    assert fwd(aux=outs["S"]) == D.E_RANGE and fwd(xout=outs["xout"], aux=outs["xout"]) == D.E_RANGE and fwd(aux=x) == D.E_RANGE
    assert fwd(xout=mis) == D.E_ALIGN and fwd(aux=mis) == D.E_ALIGN
    assert fwd(groups=5) == D.E_SHAPE and bwd(groups=5) == D.E_SHAPE
    assert fwd(dd=2052, groups=0) == D.E_RANGE and bwd(dd=2052, groups=0) == D.E_RANGE
    assert bwd(dg=None) == D.E_NULLPTR and bwd(db=None) == D.E_NULLPTR
    assert fwd(n_rows=0, xout=outs["xout"], aux=outs["aux"]) == 0 and bwd(n_rows=0) == 0
    torch.cuda.synchronize()
    for k, b in outs.items():
        assert b.untouched(), k + " was written by a call that returned before launching"
    assert mis.untouched() and not torch.isnan(x.view).any()
