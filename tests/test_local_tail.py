"""n_tail of the ODE block (graph_odenet_amd/gcn_ode.py: local_tail_rows; include/graphode.h: gode_gcn_odefunc_t.n_tail): the
length of the longest suffix of rows that are ALL isolated - their only entry in A and in A^T is their own diagonal - where
that suffix is at least 1/8 of the rows, else 0.  Hand-made graphs on the CPU, exact integer counts."""
import torch

from graph_odenet_amd import graph as G
from graph_odenet_amd.gcn_ode import CORE_LIST_MIN_SHARE_INV, local_tail_rows

N = 64


def make(n, edges, loops=None):
    """Square graph: the given off-diagonal (row, column) pairs and a self loop on every row of `loops` (default: all)."""
    loops = list(range(n)) if loops is None else list(loops)
    r = torch.tensor([e[0] for e in edges] + loops)
    c = torch.tensor([e[1] for e in edges] + loops)
    return G.from_coo(r, c, torch.full((r.numel(),), 0.5), n, n)


def ring(rows):
    """Every row of `rows` gathers the next one: none of them is isolated."""
    rows = list(rows)
    return [(a, b) for a, b in zip(rows, rows[1:] + rows[:1])]


def isolated(g):
    return (g.isolated_rows().diag != 0).nonzero().flatten().tolist()


def test_isolated_rows_that_are_not_a_suffix_give_zero():
    g = make(N, ring(range(32, N)))                       # rows 0 .. 31 isolated, the last 32 are not
    assert isolated(g) == list(range(32)) and g.isolated_tail() == 0 and local_tail_rows(g) == 0
    g = make(N, ring(list(range(16)) + [N - 1]))          # all but the last row of [16, N) isolated
    assert isolated(g) == list(range(16, N - 1)) and g.isolated_tail() == 0 and local_tail_rows(g) == 0


def test_a_suffix_shorter_than_the_gate_gives_zero():
    assert CORE_LIST_MIN_SHARE_INV == 8
    g = make(N, ring(range(N - 7)))                       # 7 of 64: 8 * 7 < 64
    assert isolated(g) == list(range(N - 7, N)) and g.isolated_tail() == 7 and local_tail_rows(g) == 0
    g = make(N, ring(range(N - 8)))                       # 8 of 64: exactly the share
    assert g.isolated_tail() == 8 and local_tail_rows(g) == 8
    g = make(N, ring(range(N - 9)))
    assert local_tail_rows(g) == 9


def test_a_suffix_plus_scattered_isolated_rows_gives_the_suffix_only():
    core = [i for i in range(40) if i % 5 != 3]           # rows 3, 8, .., 38 are isolated as well
    g = make(N, ring(core))
    assert isolated(g) == [i for i in range(40) if i % 5 == 3] + list(range(40, N))
    assert g.isolated_tail() == N - 40 and local_tail_rows(g) == N - 40
    # a row of the would-be suffix that is diagonal-only in A but gathered by somebody ends the suffix above it
    g = make(N, ring(core) + [(0, 50)])
    assert 50 not in isolated(g) and g.isolated_tail() == N - 51 and local_tail_rows(g) == N - 51
    # a row without its diagonal is not isolated either
    g = make(N, ring(core), loops=[i for i in range(N) if i != 60])
    assert g.isolated_tail() == N - 61 and local_tail_rows(g) == 0


def test_after_the_hubs_first_renumbering_the_tail_is_every_isolated_row():
    gen = torch.Generator().manual_seed(5)
    n = 300
    busy = torch.randperm(n, generator=gen)[:170].tolist()            # 130 rows keep their self loop alone, scattered
    edges = ring(busy) + [(busy[i], busy[(7 * i + 3) % 170]) for i in range(0, 170, 3) if busy[i] != busy[(7 * i + 3) % 170]]
    g = make(n, sorted(set(edges)))
    iso = isolated(g)
    assert len(iso) == 130 and g.isolated_tail() < 130
    h = g.relabel(g.degree_order())
    assert isolated(h) == list(range(n - 130, n))
    assert h.isolated_tail() == 130 and local_tail_rows(h) == 130
    assert torch.equal(h.isolated_rows().diag[n - 130:], torch.full((130,), 0.5))
