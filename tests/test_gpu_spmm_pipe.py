"""Option spmm_pipe: the thread-group SpMM that walks several tiles of records per block with the records' indices fetched
ahead (csrc/spmm.hip: spmm_vec4_pipe_kernel) against the kernel it replaces (option 0), BIT FOR BIT.

Bit identity is the derived bar, not a measured one: a lane group still owns a record and runs the same multiply-add chain
in CSR order, the same epilogue, the same slab write for a split row's records.  Only which block holds a tile, and when
its index loads are requested, changes.  The data is float (values in [0.1, 1.1), randn operands), so a changed summation
order would show.  (A launch with a cotangent output keeps the one-tile kernel under every setting, so its per-block
column sums keep their layout by construction; those cases stay here so that this stays checked should the dispatch change.)

Graphs are the designed ones of test_gpu_spmm_routes.py: L (66 003 rows: every record length the loops branch on, empty rows
beside long ones, split rows first and last), Lnr (its rowptr form) and B1 (65 537 records, the smallest size on this
route).  Widths 16, 128, 256 = lane groups of 4, 32, 64 with 64, 8, 4 records per tile.  Settings: 1 (the default: tiles per
block chosen by the launch - 1, 2 or 4 at these sizes), 3 and 5 tiles per block (neither divides a tile count here, so
some blocks walk one tile fewer than the others) and 64 (cut to what the block's LDS holds: 16 tiles at d = 16).
"""
import functools

import pytest
import torch

from test_gpu_spmm_routes import assert_route, dev, gpu_graph, profile, spmm_save

gpu = pytest.mark.gpu

SETTINGS = (1, 3, 5, 64)
KINDS = ("L", "Lnr", "B1")
WIDTHS = (16, 128, 256)
EPILOGUES = {
    "plain": dict(),
    "full": dict(bias=True, relu=True, alpha=-0.37, n_pre=2, n_cot=2, third=True, colsum=True),
    "alias": dict(bias=True, relu=True, alpha=0.25, n_pre=1, alias=True),
    "cot8": dict(bias=True, n_cot=8, colsum=True),
    "save": dict(save=True, bias=True, relu=True, alpha=-2.0, n_pre=2),
}
CASES = [(k, d, e) for k in KINDS for d in WIDTHS for e in EPILOGUES]


@functools.lru_cache(maxsize=4)
def operands(rows, cols, d):
    """randn operands of an (rows x cols) graph at width d, on the GPU: X, bias, 2 pre-terms, 8 cot-terms."""
    gen = torch.Generator(device=dev()).manual_seed(31 * d + rows)
    r = lambda *shape: torch.randn(*shape, generator=gen, device=dev())
    return r(cols, d), r(d), [r(rows, d) for _ in range(2)], [r(rows, d) for _ in range(8)]


PRE_C = [1.0, -0.7]          # the alias close has coefficient 1.0 on the array it overwrites
COT_C = [-1.3, 0.6, 0.9, -0.35, 0.15, 1.7, -0.55, 0.8]
COT3_C = [0.45, -1.1, 0.3, 0.2, -0.6, 1.2, 0.7, -0.25]


def run(kind, d, setting, bias=False, relu=False, alpha=1.0, n_pre=0, n_cot=0, third=False, colsum=False, alias=False,
        save=False):
    """One launch under spmm_pipe = setting; every array it writes, as a dict of fresh tensors."""
    from graph_odenet_amd import _lib, ops
    lib = _lib.load()
    g = gpu_graph(kind, "float")
    n = g.n_rows
    X, b, pre_t, cot_t = operands(n, g.n_cols, d)
    pre = [(c, t.clone()) for c, t in zip(PRE_C[:n_pre], pre_t)]
    cot = [(c, t) for c, t in zip(COT_C[:n_cot], cot_t)]
    out = pre[0][1] if alias else torch.full((n, d), 77.0, device=dev())
    res = {}
    old = lib.gode_get_option(b"spmm_pipe")
    try:
        assert lib.gode_set_option(b"spmm_pipe", setting) == 0 and lib.gode_get_option(b"spmm_pipe") == setting
        if save:
            res["K"] = torch.full((n, d), 77.0, device=dev())
            spmm_save(g, X, out, res["K"], b if bias else None, relu, alpha, pre)
        else:
            kw = {}
            if colsum:
                rows = ops.spmm_y2_colsum_rows(g, d)
                assert rows == (g.n_items * (d // 4) + 255) // 256 + (g.n_long * (d // 4) + 255) // 256
                res["colsum"] = kw["out2_colsum"] = torch.full((rows, d), 77.0, device=dev())
            if third:
                res["Y3"] = torch.full((n, d), 77.0, device=dev())
                kw.update(cot_out=res["Y3"], cot_out_coefs=COT3_C[:n_cot])
            if cot:
                res["Y2"] = kw["out2"] = torch.full((n, d), 77.0, device=dev())
            ops.spmm(g, X, bias=b if bias else None, relu=relu, out=out, alpha=alpha, pre_terms=pre or None,
                     cot_terms=cot or None, **kw)
        torch.cuda.synchronize()
    finally:
        lib.gode_set_option(b"spmm_pipe", old)
    res["Y"] = out
    return res


@gpu
@pytest.mark.parametrize("kind,d,epilogue", CASES, ids=["%s-%d-%s" % c for c in CASES])
def test_pipe_equals_one_tile_per_block_bit_for_bit(kind, d, epilogue):
    from graph_odenet_amd import ops
    g = gpu_graph(kind, "float")
    assert ops.spmm_y2_colsum_rows(g, d) > 0                          # the thread-group route
    assert (g.items is None) == kind.endswith("nr")
    kw = EPILOGUES[epilogue]
    want = run(kind, d, 0, **kw)
    assert not bool((want["Y"] == 77.0).all(1).any()), "the yardstick left a row unwritten"
    for setting in SETTINGS:
        got = run(kind, d, setting, **kw)
        assert got.keys() == want.keys()
        for name in want:
            if not torch.equal(got[name], want[name]):
                bad = torch.nonzero(got[name] != want[name])
                raise AssertionError("spmm_pipe %d, %s: %d of %d elements differ from spmm_pipe 0, first at %s"
                                     % (setting, name, bad.shape[0], want[name].numel(), tuple(bad[0].tolist())))


@gpu
@pytest.mark.parametrize("setting", (0,) + SETTINGS)
def test_a_product_is_one_profiled_launch(setting):
    """One profiled launch of width d per product, whatever the setting (and the finishing launch is not profiled)."""
    from graph_odenet_amd import _lib, ops
    lib = _lib.load()
    g = gpu_graph("L", "float")
    X = operands(g.n_rows, g.n_cols, 128)[0]
    old = lib.gode_get_option(b"spmm_pipe")
    try:
        assert lib.gode_set_option(b"spmm_pipe", setting) == 0
        with profile() as widths:
            ops.spmm(g, X)
    finally:
        lib.gode_set_option(b"spmm_pipe", old)
    assert_route("tg", g, 128, widths)


def test_option_values():
    """0, 1 and 2..64 are settings; anything else is refused and leaves the option as it was."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    old = lib.gode_get_option(b"spmm_pipe")
    try:
        for v in (1, 2, 64, 0):
            assert lib.gode_set_option(b"spmm_pipe", v) == 0 and lib.gode_get_option(b"spmm_pipe") == v
        for v in (-1, 65, -8):
            assert lib.gode_set_option(b"spmm_pipe", v) != 0 and lib.gode_get_option(b"spmm_pipe") == 0
    finally:
        lib.gode_set_option(b"spmm_pipe", old)
