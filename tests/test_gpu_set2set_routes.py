"""Every route and width of the Set2Set readout kernels against a float64 restatement: the one-launch loop
(csrc/set2set.hip), the fused LSTM cell (csrc/lstm.hip) and the per-graph softmax readout (csrc/segment.hip).

The cases, the limits they bracket and the restatement (QC/set2set.py:50-75 in plain torch ops, float64, CPU) are in
tests/set2set_routes_design.py; test_set2set_routes.py checks on the CPU that every case reaches its route, that plain
float32 arithmetic stays a factor 4 inside the tolerances on every case, and that five ways the kernels could be wrong are
each rejected by the comparison used here.

Loop cases run ops.set2set_fwd / set2set_bwd (the strided ones the C ABI itself, x a column block of a NaN-filled matrix,
every output pre-filled with NaN) on segments from qc_models._Segments and compare q*_t, c_t, the gate activations and the
attention weights of EVERY step, and dx, dW_ih, dW_hh, db, with the reference; q*_0 and c_0 are exactly zero, each graph's
weights sum to 1, a graph without nodes reads r = 0 exactly, and a second run is bit-identical.

Metric and bounds.  The suite's `close` metric, max |got - ref| / max(1, max |ref|), per quantity (and per step).  Loop and
segment attention: 1e-5 forward, 2e-5 gradients (test_set2set_module_vs_reference_golden's); large-logit cases
max(that, 4 x the float32 restatement's own error), capped at 1e-4.  LSTM cell: 2e-6 forward, 4e-6 sqrt(B) backward
(test_fused_lstm_cell_vs_float64's), both times max(1, sqrt((I + H) / 400)).

Measured on an MI355X (worst case of each family, forward / gradients; profiles/set2set_routes_errors.txt has every case):
  loop, ordinary cases      1.1e-6 (gates, unsorted_h512)   / 1.7e-6 (dx, steps12_h257)
  loop, large logits        4.0e-6 (gates; bound 3.5e-5)    / 2.2e-6 (dw_ih)
  loop, strided x           1.5e-7                          / 3.4e-7
  LSTM cell                 7.0e-7 (78 x 146 x 73), 9.8e-7 at 20 x 3000 x 8 (bound 5.5e-6) / 7.9e-7, 2.4e-6 at 20 x 3000 x 8
  segment attention         4.5e-7 (r, h = 1023)            / 1.5e-6 (dx, h = 1); large logits 4.7e-8 / 5.8e-7
  Set2Set(513, 3) per-step  4.0e-7 / 8.1e-7;   Set2Set(512, 3) one launch  1.7e-7 / 6.9e-7

SET2SET_ROUTES_ERRORS=<file>: the errors of the run are written there.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import set2set_routes_design as D                                       # noqa: E402

pytestmark = pytest.mark.gpu
ERRORS = {}
NAN = float("nan")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def close(a, b, tol, what=""):
    a = a.detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel() == 0:
        return
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, "%s: max err %.3e (scale %.3e)" % (what, err, scale)


@pytest.fixture(scope="module", autouse=True)
def errors_file():
    yield
    path = os.environ.get("SET2SET_ROUTES_ERRORS")
    if path and ERRORS:
        with open(path, "w") as f:
            f.write("# error of every case and quantity against float64: max |got - ref| / max(1, max |ref|)\n")
            for name, errs in ERRORS.items():
                f.write("%-28s %s\n" % (name, " ".join("%s=%.2e" % kv for kv in errs.items())))


def check(name, errors, tol):
    ERRORS[name] = errors
    print(name, " ".join("%s=%.2e" % kv for kv in errors.items()))
    bad = D.failures(errors, tol)
    assert not bad, "%s: %s" % (name, ", ".join("%s %.3e > %.3e" % (k, errors[k], tol[k]) for k in bad))


def to_dev(t):
    return None if t is None else t.to(dev())


# ---- the one-launch loop -----------------------------------------------------------------------------------------------
def run_loop_ops(v, seg, xd, W):
    from graph_odenet_amd import ops
    w_ih, w_hh, b_ih, b_hh = W
    saved = ops.set2set_fwd(seg.segptr, seg.perm, xd, w_ih, w_hh, b_ih, b_hh, v.case.T, seg.nb)
    dx, dw_ih, dw_hh, db_ih, db_hh = ops.set2set_bwd(seg.segptr, seg.perm, xd, w_ih, w_hh, b_ih is not None, saved, to_dev(v.gout))
    return dict(zip(D.FWD_KEYS, saved), dx=dx, dw_ih=dw_ih, dw_hh=dw_hh, db_ih=db_ih, db_hh=db_hh)


def run_loop_abi(v, seg, xd, W):
    """gode_set2set_f32_fwd/_bwd themselves, as ops.set2set_fwd / set2set_bwd call them, on an x with ldx > H whose base is
    not 16-byte aligned, every output pre-filled with NaN."""
    from graph_odenet_amd import _lib, ops
    lib, ptr = _lib.load(), _lib.ptr
    w_ih, w_hh, b_ih, b_hh = W
    T, B, (N, H) = v.case.T, seg.nb, xd.shape
    assert xd.stride() == (H + D.PAD, 1) and xd.data_ptr() % 16 != 0
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=dev())                           # noqa: E731
    Wt = torch.cat([w_ih, w_hh], 1).t().contiguous()
    qs, cs, gates, att = nan(T + 1, B, 2 * H), nan(T + 1, B, H), nan(T, B, 4 * H), nan(T, N)
    _lib.check(lib.gode_set2set_f32_fwd(ptr(seg.segptr), ptr(seg.perm), ptr(xd), xd.stride(0), ptr(Wt), ptr(b_ih), ptr(b_hh), B, H, T,
                                        N, ptr(qs), ptr(cs), ptr(gates), ptr(att), _lib.stream_ptr()), "gode_set2set_f32_fwd")
    dx, DG, gout = nan(N, H), nan(T, B, 4 * H), to_dev(v.gout)
    _lib.check(lib.gode_set2set_f32_bwd(ptr(seg.segptr), ptr(seg.perm), ptr(xd), xd.stride(0), ptr(w_ih), ptr(w_hh), B, H, T, N,
                                        ptr(qs), ptr(cs), ptr(gates), ptr(att), ptr(gout), ptr(dx), ptr(DG), _lib.stream_ptr()),
               "gode_set2set_f32_bwd")
    for nm, t in (("qs", qs), ("cs", cs), ("gates", gates), ("att", att), ("dx", dx), ("DG", DG)):
        assert not torch.isnan(t).any(), nm + ": an element was not written, or a foreign column was read"
    dg2 = DG.view(T * B, 4 * H)
    dw_ih = ops.gemm(dg2, qs[:T].reshape(T * B, 2 * H), trans_a=True)
    db = ops.colsum_(torch.empty(4 * H, dtype=torch.float32, device=dev()), dg2)
    return dict(qs=qs, cs=cs, gates=gates, att=att, dx=dx, dw_ih=dw_ih, dw_hh=dw_ih[:, :H].contiguous(), db_ih=db, db_hh=db)


@pytest.mark.parametrize("case", D.LOOP_CASES, ids=repr)
def test_set2set_loop_vs_float64(case):
    from graph_odenet_amd import ops
    from graph_odenet_amd.qc_models import _Segments
    v = D.loop_inputs(case.name)
    ref = D.loop_reference64(case.name)
    H = case.H
    assert ops.set2set_supported(H)
    seg = _Segments(v.batch.to(dev()))
    assert (seg.perm is None) == case.sorted_batch and seg.nb == v.nb
    assert seg.segptr.cpu().tolist() == np.concatenate([[0], np.cumsum(case.sizes)]).tolist()
    W = [to_dev(t) for t in (v.w_ih, v.w_hh, v.b_ih, v.b_hh)]
    if case.strided:
        xd = v.xfull.to(dev())[:, 1:1 + H]
        run = run_loop_abi
    else:
        xd = v.x.to(dev())
        run = run_loop_ops
    got = run(v, seg, xd, W)
    e32 = D.loop_errors(D.loop_reference(case.name, torch.float32), ref) if case.large_logits else None
    check("loop/" + case.name, D.loop_errors(got, ref), D.tolerances(D.LOOP_TOL, e32))
    assert got["qs"][0].abs().max().item() == 0.0 and got["cs"][0].abs().max().item() == 0.0
    att = got["att"].cpu().double()
    for b, n in enumerate(case.sizes):
        if n:
            s = att[:, v.batch == b].sum(1)
            assert (s - 1.0).abs().max().item() <= 1e-6 * n, (b, n, s)
        else:                                            # r = 0 exactly; its rows of the state are the reference's
            assert got["qs"][:, b, H:].abs().max().item() == 0.0 and ref["qs"][:, b, H:].abs().max().item() == 0.0
            close(got["qs"][:, b], ref["qs"][:, b], D.TOL_FWD, "q* of the empty graph")
            close(got["cs"][:, b], ref["cs"][:, b], D.TOL_FWD, "c of the empty graph")
    again = run(v, seg, xd, W)                           # fixed summation order: bit-identical
    for k, t in got.items():
        if t is not None:
            assert torch.equal(t, again[k]), k + " differs between two runs"


# ---- the LSTM cell -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I,H", [shape for shape, _ in D.LSTM_CASES])
@pytest.mark.parametrize("bias", [True, False])
def test_fused_lstm_cell_chunks_vs_float64(B, I, H, bias):
    """test_fused_lstm_cell_vs_float64's body on the shapes that reach two and three chunks of rows, the LDS-limited chunk,
    the largest supported B at the workload's width and the smallest shape; support is asserted, not skipped on."""
    from graph_odenet_amd import ops
    from graph_odenet_amd.qc_models import _LstmCellFn
    assert ops.lstm_cell_supported(B, I, H)
    tol_f, tol_b = D.lstm_tolerances(B, I, H)
    g = torch.Generator().manual_seed(B + 3 * I + 7 * H)
    mk = lambda *s: torch.randn(*s, generator=g)                                                     # noqa: E731
    x, h, c = mk(B, I), mk(B, H), mk(B, H)
    w_ih, w_hh = mk(4 * H, I) / I ** 0.5, mk(4 * H, H) / H ** 0.5
    b_ih, b_hh = (mk(4 * H), mk(4 * H)) if bias else (None, None)
    gh, gc = mk(B, H), mk(B, H)
    for use_gc in (True, False):
        ref_in = [t.double().requires_grad_(True) if t is not None else None for t in (x, h, c, w_ih, w_hh, b_ih, b_hh)]
        rh, rc = torch.lstm_cell(ref_in[0], (ref_in[1], ref_in[2]), ref_in[3], ref_in[4], ref_in[5], ref_in[6])
        ((rh * gh.double()).sum() + ((rc * gc.double()).sum() if use_gc else 0.0)).backward()
        dev_in = [t.to(dev()).requires_grad_(True) if t is not None else None for t in (x, h, c, w_ih, w_hh, b_ih, b_hh)]
        oh, oc = _LstmCellFn.apply(*dev_in)
        errs = {"h'": D.rel_err(oh, rh), "c'": D.rel_err(oc, rc)}
        ((oh * gh.to(dev())).sum() + ((oc * gc.to(dev())).sum() if use_gc else 0.0)).backward()
        for a, b, nm in zip(dev_in, ref_in, ("dx", "dh", "dc", "dw_ih", "dw_hh", "db_ih", "db_hh")):
            if a is not None:
                errs[nm] = D.rel_err(a.grad, b.grad)
        check("lstm/%dx%dx%d%s%s" % (B, I, H, "" if bias else "/nobias", "" if use_gc else "/dh-only"), errs,
              {k: (tol_f if k in ("h'", "c'") else tol_b) for k in errs})


# ---- segment attention -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.SEG_CASES, ids=repr)
def test_segment_attention_widths_vs_float64(case):
    """test_segment_attention_vs_oracle's checks on the widths of every instantiation (MC = 8 among them) and of both sides
    of every 64-column chunk, segments of 255, 256, 257 and 1000 nodes, logits of several hundred, and an x with ldx > h."""
    from graph_odenet_amd import _lib, ops
    from graph_odenet_amd.qc_models import _Segments
    v = D.seg_inputs(case.name)
    ref = D.seg_reference(case.name)
    h, n = case.h, v.batch.numel()
    seg = _Segments(v.batch.to(dev()))
    assert (seg.perm is None) == case.sorted_batch and seg.nb == v.nb
    qd, drd = v.q.to(dev()), v.dr.to(dev())
    if not case.strided:
        xd = v.x.to(dev())
        a, r = ops.segment_attention_fwd(seg.segptr, seg.perm, xd, qd)
        dx, dq = ops.segment_attention_bwd(seg.segptr, seg.perm, xd, qd, a, drd)
    else:
        lib, ptr = _lib.load(), _lib.ptr
        xd = v.xfull.to(dev())[:, 1:1 + h]
        assert xd.stride() == (h + D.PAD, 1) and xd.data_ptr() % 16 != 0
        nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=dev())                       # noqa: E731
        a, r, dx, dq = nan(n), nan(v.nb, h), nan(n, h), nan(v.nb, h)
        _lib.check(lib.gode_segment_attention_f32_fwd(ptr(seg.segptr), ptr(seg.perm), ptr(xd), xd.stride(0), ptr(qd), v.nb, h, ptr(a),
                                                      ptr(r), _lib.stream_ptr()), "gode_segment_attention_f32_fwd")
        _lib.check(lib.gode_segment_attention_f32_bwd(ptr(seg.segptr), ptr(seg.perm), ptr(xd), xd.stride(0), ptr(qd), ptr(a), ptr(drd),
                                                      v.nb, h, ptr(dx), ptr(dq), _lib.stream_ptr()), "gode_segment_attention_f32_bwd")
        for nm, t in (("a", a), ("r", r), ("dx", dx), ("dq", dq)):
            assert not torch.isnan(t).any(), nm + ": an element was not written, or a foreign column was read"
    e32 = D.seg_errors(D.seg_reference(case.name, torch.float32), ref) if case.large_logits else None
    check("segment/" + case.name, D.seg_errors(dict(a=a, r=r, dx=dx, dq=dq), ref), D.tolerances(D.SEG_TOL, e32))
    ac = a.cpu().double()
    for b, nodes in enumerate(case.sizes):
        if nodes:
            assert abs(ac[v.batch == b].sum().item() - 1.0) <= 1e-6 * nodes
        else:
            assert r[b].abs().max().item() == 0.0 and dq[b].abs().max().item() == 0.0


# ---- module level ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,path", D.MODULE_CASES)
def test_set2set_module_at_the_loop_kernels_width_limit(channels, path):
    """Set2Set(512, 3) is the widest the one-launch loop takes; Set2Set(513, 3) goes to the per-step path (the loop refuses
    it, the fused LSTM cell takes its 7 graphs, the segment attention runs MC = 16).  Both against float64, through autograd."""
    from graph_odenet_amd import ops
    from graph_odenet_amd.qc_models import Set2Set
    v, ref = D.module_inputs(channels), D.module_reference(channels)
    nb, batch, x, gout = v.nb, v.batch, v.x, v.gout
    w_ih, w_hh, b_ih, b_hh = v.w_ih, v.w_hh, v.b_ih, v.b_hh
    assert ops.set2set_supported(channels) == (path == "one-launch")
    assert ops.lstm_cell_supported(nb, 2 * channels, channels)
    m = Set2Set(channels, 3)
    m.lstm.load_state_dict({"weight_ih_l0": w_ih, "weight_hh_l0": w_hh, "bias_ih_l0": b_ih, "bias_hh_l0": b_hh})
    m = m.to(dev())
    xd = x.to(dev()).requires_grad_(True)
    out = m(xd, batch.to(dev()))
    assert type(out.grad_fn).__name__ == ("_Set2SetFnBackward" if path == "one-launch" else "CatBackward0")
    out.backward(gout.to(dev()))
    errs = {"qs": D.rel_err(out, ref["qs"][3]), "dx": D.rel_err(xd.grad, ref["dx"])}
    for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
        errs["d" + k] = D.rel_err(getattr(m.lstm, {"w": "weight_", "b": "bias_"}[k[0]] + k[2:] + "_l0").grad, ref["d" + k])
    check("module/Set2Set(%d,3)" % channels, errs, {k: (D.TOL_FWD if k == "qs" else D.TOL_GRAD) for k in errs})
