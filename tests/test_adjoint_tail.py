"""A's record list without the isolated tail rows (graph_odenet_amd/gcn_ode.py: head_items; include/graphode.h:
gode_gcn_odefunc_t.a_head_items), the list Sp(g) of the adjoint solve walks under option adjoint_tail: its gate and its
contents, from exact integer counts on the CPU."""
import torch

from graph_odenet_amd import gcn_ode
from graph_odenet_amd import graph as G
from graph_odenet_amd.synth import rmat_graph

MIN_ROWS = gcn_ode.CORE_LIST_MIN_ROWS


def chain_graph(n_core, n_tail, split=256):
    """Rows 0 .. n_core - 1 gather their successor (a ring: none is isolated) and every row has its self loop; row 0 is long
    enough to be split into several records.  The last n_tail rows hold their self loop alone."""
    n = n_core + n_tail
    ar = torch.arange(n_core)
    hub = torch.arange(1, 3 * split)
    r = torch.cat([ar, torch.zeros_like(hub), torch.arange(n)])
    c = torch.cat([(ar + 1) % n_core, hub + 1, torch.arange(n)])
    key = torch.unique(r * n + c)
    return G.from_coo(key // n, key % n, torch.full((key.numel(),), 0.5), n, n, split=split, coalesce=False)


def tuned(g):
    tg, order, _ = gcn_ode.tuned_graph(g, 128, node_order="given")
    assert tg is g and order is None
    return g.__dict__["_tuned_info"][(128, "given")]


def test_the_list_is_the_records_of_the_rows_before_the_tail_in_order():
    n_core, n_tail = MIN_ROWS + 37, 20_000
    g = chain_graph(n_core, n_tail)
    info = tuned(g)
    assert info["core_lists"] and info["n_tail"] == n_tail and g.__dict__["_n_tail"] == n_tail
    head = g.__dict__["_a_head"]
    assert head is not None and head.dtype == torch.int32 and head.is_contiguous()
    keep = g.items[:, 0] < n_core
    assert int((~keep).sum()) == n_tail                               # a tail row is one record
    assert torch.equal(head, g.items[keep])                           # the same records in the same order
    assert head.shape[0] == g.n_items - n_tail == info["head_records"]
    assert g.n_long == 1 and int((head[:, 3] >= 0).sum()) == g.n_slots == 4       # the split row keeps all its records
    fs = gcn_ode._func_struct(gcn_ode.GcnOdeSpec(g, torch.zeros(129, 128), torch.zeros(128), torch.ones(128), torch.zeros(128), 32, 1e-5))
    assert fs.n_tail == n_tail and fs.a_n_head == head.shape[0] and fs.a_head_items == head.data_ptr()


def test_absent_without_a_tail():
    # the isolated rows are there (a quarter of the rows) but the last row is not one of them: n_tail = 0
    n_core, n_iso = MIN_ROWS + 37, 30_000
    n = n_core + n_iso
    ar = torch.arange(n_core)
    rows = torch.cat([ar[:-1], torch.tensor([n - 1])])                # the ring's last member sits behind the isolated rows
    r = torch.cat([rows, torch.arange(n)])
    c = torch.cat([rows.roll(-1), torch.arange(n)])
    g = G.from_coo(r, c, torch.full((r.numel(),), 0.5), n, n, split=256)
    info = tuned(g)
    assert info["core_lists"] and info["isolated_rows"] == n_iso + 1 - 1 and info["n_tail"] == 0
    assert g.__dict__["_a_head"] is None and info["head_records"] == 0
    fs = gcn_ode._func_struct(gcn_ode.GcnOdeSpec(g, torch.zeros(129, 128), torch.zeros(128), torch.ones(128), torch.zeros(128), 32, 1e-5))
    assert fs.n_tail == 0 and fs.a_n_head == 0 and not fs.a_head_items


def test_absent_below_an_eighth_of_the_rows():
    n_core = MIN_ROWS + 64
    below = n_core // 7 - 1                                           # 8 * below < n_core + below
    assert 8 * below < n_core + below
    g = chain_graph(n_core, below)
    info = tuned(g)
    assert not info["core_lists"] and info["n_tail"] == 0 and g.__dict__["_a_head"] is None
    at = (n_core + 6) // 7                                            # the smallest tail with 8 * tail >= n
    assert 8 * at >= n_core + at and 8 * (at - 1) < n_core + at - 1
    g = chain_graph(n_core, at)
    info = tuned(g)
    assert info["n_tail"] == at and g.__dict__["_a_head"].shape[0] == g.n_items - at


def test_absent_with_at_most_65536_rows_before_the_tail():
    for n_core, want in ((MIN_ROWS, False), (MIN_ROWS + 1, True)):
        g = chain_graph(n_core, 20_000)
        info = tuned(g)
        assert info["core_lists"] and info["n_tail"] == 20_000        # the forward solve's tail is there either way
        assert (g.__dict__["_a_head"] is not None) is want
        assert gcn_ode.head_items(g, 20_000) is None or want


def test_rmat_17_under_degree_order():
    """The problem of tests/test_gpu_large_adjoint.py: the route engages there (53 623 tail rows, 77 449 before them)."""
    g0 = rmat_graph(17, 1 << 20, seed=1)
    g = g0.relabel(g0.degree_order())                                 # what node_order = "degree" integrates on
    info = tuned(g)
    assert info["n_tail"] == 53_623 == info["isolated_rows"] and g.n_rows - info["n_tail"] == 77_449 > MIN_ROWS
    head = g.__dict__["_a_head"]
    assert head is not None and head.shape[0] == g.n_items - 53_623 == info["head_records"]
    assert int(head[:, 0].max()) == 77_448
    assert torch.equal(head, g.items[g.items[:, 0] < 77_449])
