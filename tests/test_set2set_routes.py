"""The design of the Set2Set readout route tests, checked on the CPU: every case of set2set_routes_design.py reaches the
route its entry names (recomputed here from the design's written-out limits), the tables together reach every route, the
support boundaries answer through the C ABI (host-side checks that launch nothing, so the pointers are made up), a float32
restatement of the reference stays inside the GPU tests' tolerances on every case (the inputs are conditioned well enough
for those tolerances to mean something), and five deliberately altered copies of the float64 restatement are each rejected
by the very comparison the GPU tests use.  No GPU.
"""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import set2set_routes_design as D                                       # noqa: E402

from graph_odenet_amd import _lib                                       # noqa: E402

P = {name: 0x10000 * (k + 1) for k, name in enumerate(
    ("segptr", "perm", "x", "wt", "b_ih", "b_hh", "qs", "cs", "gates", "att", "w_ih", "w_hh", "dq", "dx", "dg", "q", "a", "r", "dr"))}


def vp(name):
    return ctypes.c_void_p(P[name])


# ---- routes ------------------------------------------------------------------------------------------------------------
def test_limits_are_the_sources():
    """The numbers the design states are the ones in the kernels' sources."""
    root = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    s2s, lstm, seg = (open(os.path.join(root, f)).read() for f in ("set2set.hip", "lstm.hip", "segment.hip"))
    assert "constexpr int NT = %d, kWaves = NT / %d;" % (D.NT, D.LANES) in s2s
    assert "constexpr int kXCap = %d;" % D.XCAP in s2s
    assert "return H > 0 && H <= %d;" % D.S2S_HMAX in s2s and "steps > %d" % D.S2S_STEPS_MAX in s2s
    assert "constexpr int kLstmMaxLds = %d;" % D.LSTM_LDS in lstm and "if (cb > %d) cb = %d;" % (D.LSTM_ROWS, D.LSTM_ROWS) in lstm
    assert "if (h > %d) return GODE_E_UNSUPPORTED;" % D.SEG_HMAX in seg and "__launch_bounds__(%d)" % D.SEG_THREADS in seg
    for m in D.SEG_MCS:
        assert "KERNEL<%d>" % m in seg
    header = " ".join(open(_lib.HEADER_PATH).read().split())
    for name, value in (("NULLPTR", D.E_NULLPTR), ("SHAPE", D.E_SHAPE), ("RANGE", D.E_RANGE), ("UNSUPPORTED", D.E_UNSUPPORTED)):
        assert "#define GODE_E_%s (%d)" % (name, value) in header


@pytest.mark.parametrize("case", D.LOOP_CASES, ids=repr)
def test_every_loop_case_reaches_its_route(case):
    assert D.set2set_supported(case.H)
    got = D.loop_route(case.H, case.sizes, case.sorted_batch)
    assert case.reaches <= got, (case.name, case.reaches - got)
    assert case.sizes[-1] > 0                      # the largest graph id has nodes: the batch vector names every graph
    assert sum(case.sizes) <= 25_000 and sum(case.sizes) * case.H <= 70_000 and 12 * case.H * case.H <= 3_200_000      # nothing needs the workload's sizes


def test_width_table_is_the_issues():
    by = {c.name: c for c in D.LOOP_CASES}
    for H in (1, 3, 16, 63, 64, 65, 73, 128, 129, 255, 256, 257, 300, 511, 512):
        c = by["width%d" % H]
        assert c.T == 3 and c.bias and c.sorted_batch and not c.strided and c.xscale == 1.0
        assert c.sizes[:7] == [1, 0, 2, 15, 16, 17, 33] and c.sizes[7:] == [12288 // H, 12288 // H + 1]
        assert c.sizes[7] * H <= 12288 < c.sizes[8] * H
    # the k-split counts of matvec_cols the table was chosen for (threads per slice, slices, passes, last pass, idle)
    assert D.matvec_route(4 * 1) == (64, 16, 1, 4, 0) and D.matvec_route(4 * 16) == (64, 16, 1, 64, 0)
    assert D.matvec_route(4 * 73) == (320, 3, 1, 292, 64)
    assert D.matvec_route(4 * 129) == (576, 1, 1, 516, 448)
    assert D.matvec_route(4 * 255) == (1024, 1, 1, 1020, 0) and D.matvec_route(4 * 256) == (1024, 1, 1, 1024, 0)
    assert D.matvec_route(4 * 257) == (1024, 1, 2, 4, 0) and D.matvec_route(4 * 300) == (1024, 1, 2, 176, 0)
    assert D.matvec_route(4 * 511) == (1024, 1, 2, 1020, 0) and D.matvec_route(4 * 512) == (1024, 1, 2, 1024, 0)
    assert D.matvec_route(2 * 512) == (1024, 1, 1, 1024, 0)             # the backward's widest product
    for H, Ts in ((73, (1, 2, 12)), (257, (1, 2, 12))):
        assert [by["steps%d_h%d" % (T, H)].T for T in Ts] == list(Ts)
    assert all(not by["unsorted_h%d" % H].sorted_batch for H in (16, 73, 257, 512))
    assert not by["nobias_h73"].bias and not by["nobias_h300"].bias
    assert by["large_logits"].T == 2 and by["large_logits"].H == 73 and by["large_logits"].xscale == 30.0
    assert by["strided_h73"].strided and by["strided_h16"].strided


def test_tables_reach_every_route_sorted_and_unsorted():
    reached = {True: set(), False: set()}
    for c in D.LOOP_CASES:
        reached[c.sorted_batch] |= D.loop_route(c.H, c.sizes, c.sorted_batch)
    for s in (True, False):
        for tag in ("staged", "unstaged", "passes1", "passes2", "4H==NT", "over1024", "empty", "wave_trips>1"):
            assert tag in reached[s], (s, tag)
    both = reached[True] | reached[False]
    for tag in ("kslices16", "kslices4", "kslices3", "kslices2", "kslices1", "idle_threads", "partial_last_pass", "2H==NT",
                "one_graph", "unstaged_first_last"):
        assert tag in both, tag
    # a third pass of matvec_cols does not exist inside the supported range: 4H <= 2048 = 2 NT for every H <= 512
    assert max(D.matvec_route(4 * H)[2] for H in range(1, D.S2S_HMAX + 1)) == 2
    assert D.matvec_route(4 * (D.S2S_HMAX + 1))[2] == 3 and not D.set2set_supported(D.S2S_HMAX + 1)
    strided = [c for c in D.LOOP_CASES if c.strided]
    assert all("unstaged" in D.loop_route(c.H, c.sizes, c.sorted_batch) for c in strided) and {c.H for c in strided} == {16, 73}
    # segment attention: every instantiation, sorted and unsorted; both sides of every chunk boundary; long segments
    for s in (True, False):
        assert {c.mc for c in D.SEG_CASES if c.sorted_batch == s and not c.large_logits} == set(D.SEG_MCS)
    assert {h: D.seg_mc(h) for h in D.SEG_WIDTHS} == {1: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 300: 8, 512: 8,
                                                      513: 16, 1023: 16}
    assert {255, 256, 257, 1000} <= set(D.SEG_SIZES) and 0 in D.SEG_SIZES and max(D.SEG_SIZES) > 3 * D.SEG_THREADS
    assert any(c.strided for c in D.SEG_CASES) and any(c.large_logits for c in D.SEG_CASES)
    # the LSTM cell: 1, 2 and 3 chunks of rows, the LDS-limited chunk, the largest B at the workload's width
    chunks = {shape: D.lstm_chunks(*shape) for shape, _ in D.LSTM_CASES}
    assert chunks[(1, 1, 1)] == (1, 1, False) and chunks[(65, 32, 16)] == (64, 2, False) and chunks[(128, 32, 16)] == (64, 2, False)
    assert chunks[(130, 32, 16)] == (64, 3, False) and chunks[(20, 3000, 8)] == (4, 5, True) and chunks[(78, 146, 73)] == (64, 2, False)
    assert all(D.lstm_supported(*shape) for shape, _ in D.LSTM_CASES)
    assert D.lstm_supported(78, 146, 73) and not D.lstm_supported(79, 146, 73)
    # module level: 513 is refused by the loop and taken by the cell with these 7 graphs; 512 is the loop's
    nb = len(D.MODULE_SIZES)
    assert not D.set2set_supported(513) and D.lstm_supported(nb, 2 * 513, 513) and not D.lstm_supported(nb + 1, 2 * 513, 513)
    assert D.set2set_supported(512) and D.seg_mc(513) == 16


# ---- support boundaries through the ABI ----------------------------------------------------------------------------------
def s2s_fwd(H, steps=3, ldx=None, n_graphs=4, n_nodes=40):
    return _lib.load().gode_set2set_f32_fwd(vp("segptr"), vp("perm"), vp("x"), H if ldx is None else ldx, vp("wt"), vp("b_ih"),
                                            vp("b_hh"), n_graphs, H, steps, n_nodes, vp("qs"), vp("cs"), vp("gates"), vp("att"), None)


def s2s_bwd(H, steps=3, ldx=None, n_graphs=4, n_nodes=40):
    return _lib.load().gode_set2set_f32_bwd(vp("segptr"), vp("perm"), vp("x"), H if ldx is None else ldx, vp("w_ih"), vp("w_hh"),
                                            n_graphs, H, steps, n_nodes, vp("qs"), vp("cs"), vp("gates"), vp("att"), vp("dq"),
                                            vp("dx"), vp("dg"), None)


def test_support_boundaries_through_the_abi():
    lib = _lib.load()
    assert lib.gode_set2set_supported(512) == 1 and lib.gode_set2set_supported(513) == 0 and lib.gode_set2set_supported(0) == 0
    assert lib.gode_set2set_supported(1) == 1 and lib.gode_set2set_supported(-1) == 0
    assert lib.gode_lstm_cell_supported(78, 146, 73) == 1 and lib.gode_lstm_cell_supported(79, 146, 73) == 0
    for (B, I, H), _ in D.LSTM_CASES:
        assert lib.gode_lstm_cell_supported(B, I, H) == 1
    for B in range(1, 12):                                   # the written-out rule is the library's, at the module case's width
        assert bool(lib.gode_lstm_cell_supported(B, 1026, 513)) == D.lstm_supported(B, 1026, 513)
    for f in (s2s_fwd, s2s_bwd):
        assert f(73, ldx=72) == D.E_SHAPE and f(73, steps=0) == D.E_SHAPE and f(73, steps=-1) == D.E_SHAPE
        assert f(513) == D.E_UNSUPPORTED
        assert f(73, steps=D.S2S_STEPS_MAX + 1) == D.E_RANGE
        assert f(73, n_graphs=0) == 0                         # nothing to launch
    assert lib.gode_segment_attention_f32_fwd(vp("segptr"), vp("perm"), vp("x"), 1025, vp("q"), 4, 1025, vp("a"), vp("r"),
                                              None) == D.E_UNSUPPORTED
    assert lib.gode_segment_attention_f32_bwd(vp("segptr"), vp("perm"), vp("x"), 1025, vp("q"), vp("a"), vp("dr"), 4, 1025,
                                              vp("dx"), vp("dq"), None) == D.E_UNSUPPORTED
    assert lib.gode_segment_attention_f32_fwd(vp("segptr"), vp("perm"), vp("x"), 72, vp("q"), 4, 73, vp("a"), vp("r"), None) == D.E_SHAPE


# ---- the reference and the conditioning of the inputs ------------------------------------------------------------------
def test_restatement_agrees_with_torch_lstm_cell_and_softmax():
    """The written-out cell against torch.lstm_cell and the segment softmax against torch.softmax per graph, float64."""
    v = D.loop_inputs("width16")
    ref = D.loop_reference64("width16")
    H, nb = 16, v.nb
    f = lambda t: t.double()                                                                         # noqa: E731
    h, c = torch.zeros(nb, H, dtype=torch.float64), torch.zeros(nb, H, dtype=torch.float64)
    q_star = torch.zeros(nb, 2 * H, dtype=torch.float64)
    for t in range(v.case.T):
        h, c = torch.lstm_cell(q_star, (h, c), f(v.w_ih), f(v.w_hh), f(v.b_ih), f(v.b_hh))
        e = (f(v.x) * h[v.batch]).sum(-1)
        a = torch.zeros_like(e)
        for b in range(nb):
            m = v.batch == b
            a[m] = torch.softmax(e[m], 0)
        r = torch.zeros(nb, H, dtype=torch.float64).index_add(0, v.batch, a[:, None] * f(v.x))
        q_star = torch.cat([h, r], -1)
        assert D.rel_err(ref["qs"][t + 1], q_star) < 1e-14 and D.rel_err(ref["cs"][t + 1], c) < 1e-14
        assert D.rel_err(ref["att"][t], a) < 1e-14
    assert ref["qs"][0].abs().max() == 0 and ref["cs"][0].abs().max() == 0
    assert ref["qs"][:, 1, H:].abs().max() == 0                      # the graph without nodes: r = 0
    assert D.rel_err(ref["dw_hh"], ref["dw_ih"][:, :H]) < 1e-14       # h_{t-1} is the left half of q*_{t-1}


@pytest.mark.parametrize("case", D.LOOP_CASES, ids=repr)
def test_float32_restatement_stays_inside_the_loop_budget(case):
    ref = D.loop_reference64(case.name)
    e32 = D.loop_errors(D.loop_reference(case.name, torch.float32), ref)
    if case.large_logits:
        assert ref["logits"].abs().max().item() >= 100.0            # past expf's overflow without the max-subtraction
        assert all(4.0 * e <= D.TOL_CAP for e in e32.values()), e32
        tol = D.tolerances(D.LOOP_TOL, e32)
        assert all(tol[k] >= max(D.LOOP_TOL[k], 4.0 * e32[k]) for k in tol)
    else:
        # the factor 4 of the large-logit rule: room for the kernels' other summation order and the device's expf / tanhf
        assert all(4.0 * e <= D.LOOP_TOL[k] for k, e in e32.items()), e32
    assert not D.failures(e32, D.tolerances(D.LOOP_TOL, e32 if case.large_logits else None))


@pytest.mark.parametrize("case", D.SEG_CASES, ids=repr)
def test_float32_restatement_stays_inside_the_segment_budget(case):
    ref = D.seg_reference(case.name)
    e32 = D.seg_errors(D.seg_reference(case.name, torch.float32), ref)
    if case.large_logits:
        assert ref["logits"].abs().max().item() >= 200.0
        assert all(4.0 * e <= D.TOL_CAP for e in e32.values()), e32
    else:
        assert all(4.0 * e <= D.SEG_TOL[k] for k, e in e32.items()), e32
    v = D.seg_inputs(case.name)
    assert ref["r"][2].abs().max() == 0 and ref["dq"][2].abs().max() == 0          # the graph without nodes
    assert (v.xfull is not None) == case.strided


@pytest.mark.parametrize("channels,path", D.MODULE_CASES)
def test_float32_restatement_stays_inside_the_module_budget(channels, path):
    e32 = D.loop_errors(D.module_reference(channels, torch.float32), D.module_reference(channels))
    assert all(4.0 * e <= D.LOOP_TOL[k] for k, e in e32.items()), e32
    assert D.module_inputs(channels).x.shape == (sum(D.MODULE_SIZES), channels)


def test_lstm_tolerances():
    assert D.lstm_tolerances(64, 146, 73) == (2e-6, 4e-6 * 8.0) and D.lstm_tolerances(7, 300, 100) == (2e-6, 4e-6 * 7 ** 0.5)
    f, b = D.lstm_tolerances(20, 3000, 8)
    assert math.isclose(f, 2e-6 * (3008 / 400) ** 0.5) and math.isclose(b, 4e-6 * 20 ** 0.5 * (3008 / 400) ** 0.5)


def test_strided_inputs_are_surrounded_by_nan():
    for name in ("strided_h73", "strided_h16"):
        v = D.loop_inputs(name)
        H = v.case.H
        assert v.x.stride(0) == H + D.PAD and v.x.storage_offset() == 1 and not v.x.is_contiguous()
        assert torch.isnan(v.xfull[:, 0]).all() and torch.isnan(v.xfull[:, 1 + H:]).all() and torch.isfinite(v.x).all()
        assert torch.equal(D.rows_as_read(v), v.x)


# ---- sensitivity: altered copies of the restatement under the GPU test's comparison ----------------------------------------
def rejected(name, fault, dtype=torch.float64):
    case = D.LOOP_BY_NAME[name]
    ref = D.loop_reference64(name)
    e32 = D.loop_errors(D.loop_reference(name, torch.float32), ref) if case.large_logits else None
    return D.failures(D.loop_errors(D.loop_reference(name, dtype, fault), ref), D.tolerances(D.LOOP_TOL, e32))


def test_gate_rows_past_1024_left_at_their_bias_are_rejected():
    bad = rejected("width257", "gate_rows_past_1024_at_bias")
    assert "gates" in bad and "qs" in bad and "dw_ih" in bad
    assert rejected("width300", "gate_rows_past_1024_at_bias") and rejected("unsorted_h512", "gate_rows_past_1024_at_bias")
    assert not rejected("width256", "gate_rows_past_1024_at_bias")               # no such row: the widths above 256 are needed


def test_unnormalised_weights_past_node_1024_are_rejected():
    for name in ("n1100_h8_sorted", "n1100_h8_unsorted", "n1100_h16_sorted", "n1100_h16_unsorted", "width1"):
        assert "att" in rejected(name, "weights_past_1024_unnormalised"), name
    assert not rejected("width73", "weights_past_1024_unnormalised")             # no graph that long: the long graphs are needed


def test_unstaged_rows_read_with_stride_h_are_rejected():
    for name in ("strided_h73", "strided_h16"):
        v = D.loop_inputs(name)
        alt = D.rows_as_read(v, unstaged_stride=v.case.H)
        big = torch.tensor([s * v.case.H > D.XCAP for s in v.case.sizes])[v.batch]
        assert big.any() and torch.equal(alt[~big], v.x[~big]) and not torch.equal(alt[big], v.x[big])
        assert rejected(name, "unstaged_rows_stride_h"), name


def test_softmax_without_max_subtraction_is_not_finite_on_the_large_logits():
    res = D.loop_reference("large_logits", torch.float32, "no_max_subtraction")
    assert not torch.isfinite(res["att"]).all() and not torch.isfinite(res["qs"]).all()
    assert set(rejected("large_logits", "no_max_subtraction", torch.float32)) >= {"qs", "att", "dx"}
    # and on ordinary logits the same alteration is invisible: the large-logit case is needed
    assert not D.failures(D.loop_errors(D.loop_reference("width73", torch.float32, "no_max_subtraction"),
                                        D.loop_reference64("width73")), D.LOOP_TOL)


def test_dw_hh_from_the_wrong_columns_is_rejected():
    for name in ("width1", "width73", "width512"):
        assert rejected(name, "dw_hh_from_wrong_columns") == ["dw_hh"], name


def test_comparison_rejects_nan_shape_and_one_entry():
    ref = D.loop_reference64("width3")
    got = {k: (None if v is None else v.clone()) for k, v in ref.items()}
    assert not D.failures(D.loop_errors(got, ref), D.LOOP_TOL)
    got["cs"][2, 3, 1] += 3e-5
    assert D.failures(D.loop_errors(got, ref), D.LOOP_TOL) == ["cs"]
    got["cs"][2, 3, 1] = float("nan")
    assert D.failures(D.loop_errors(got, ref), D.LOOP_TOL) == ["cs"]
    got["cs"] = ref["cs"][:, :, :2]
    assert D.failures(D.loop_errors(got, ref), D.LOOP_TOL) == ["cs"]
