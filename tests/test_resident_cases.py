"""tests/resident_cases.py on the CPU: every entry builds with the counts it names, the restated dynamic-LDS
bytes of each "fit" entry are exactly the budget (or half of it) and those of each "over" entry one step
above, every edge has an entry on each side, and the float64 oracle keeps the entries well conditioned."""
import numpy as np
import pytest

from tests import resident_cases as rc
from tests import shape_cases as sc

SMALL = sorted(rc.CASES) + sorted(rc.GROUPED)
ALL = SMALL + sorted(rc.ROWS16)


@pytest.mark.parametrize("name", ALL)
def test_entry_builds_with_the_requested_counts(name):
    """The generator's contract on every built graph, as test_shape_cases.py holds the shape table to it."""
    c = rc.case(name)
    _, _, _, plan, graphs, labels, _ = rc.case_inputs(name)
    assert plan.hidden == [32] * len(plan.entities) and plan.iterations == sc.ITERATIONS
    for spec, g, y in zip(c.graphs, graphs, labels):
        a = dict(spec)
        lens = np.asarray(a["lens"])
        P, L = a["P"], a["L"] + a.get("idle_links", 0)
        assert (g["num_path"], g["num_link"], y.size) == (P, L, P)
        assert g["traffic"].shape == (P,) and g["link_capacity"].shape == (L,)
        assert g["traffic"].dtype == np.float32 and np.abs(g["traffic"]).max() <= 1
        dst, src, seq = (np.asarray(g[k]) for k in ("dst_adj_links_paths", "src_adj_links_paths", "seq_link_path"))
        np.testing.assert_array_equal(np.bincount(dst, minlength=P), lens)
        deg = np.bincount(src, minlength=L)
        np.testing.assert_array_equal(deg, np.bincount(g["dst_adj_paths_links"], minlength=L))
        assert np.all(deg[a["L"]:] == 0) and np.all(deg[1:a["L"]] >= 1)
        if "hot" in a:
            assert deg[0] == a["hot"]
        # per path: positions 0 .. len - 1 once each, over distinct links (dst is path-sorted)
        assert np.all(np.diff(dst) >= 0)
        first = np.concatenate([[0], np.cumsum(lens)[:-1]])
        np.testing.assert_array_equal(seq, np.arange(dst.size) - np.repeat(first, lens))
        pairs = dst * L + src
        assert np.unique(pairs).size == pairs.size
        if c.kind == "qsize":
            assert g["num_node"] == a["N"] and g["queue_sizes"].shape == (a["N"],)
            np.testing.assert_array_equal(np.bincount(g["dst_adj_nodes_paths"], minlength=P), lens)
            assert np.all(np.bincount(g["src_adj_nodes_paths"], minlength=a["N"]) >= 1)
            assert len(g["indices_link_to_path"]) == len(g["indices_node_to_path"]) == lens.max()


def test_worked_example():
    """The issue's first entry by hand: 5 links, 902 paths, 891 of length 4 and 11 of length 3."""
    (g,) = rc.case_inputs("a_fit")[4]
    c = rc.counts([g], "routenet")
    assert c == rc.Counts(U=5, M=3597, P=902, C=3609, tiles=1)
    assert [rc.lds_bytes(c, f) for f in range(3)] == [3156 + 7194 + 129888 + 7218, 3156 + 7194, 3156]
    assert rc.lds_bytes(c, 0) == rc.LIMIT == 147456


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_entry_sits_where_it_says(name):
    """A "fit" entry's deciding bytes are exactly the budget (edges A and B), half of it (D), or those of the
    last union-row count that fits (C); an "over" entry is one step above: 4 bytes, one message (2 bytes,
    edge B) or one union row (C)."""
    c = rc.case(name)
    graphs = rc.case_inputs(name)[4]
    e = rc.case_expected(name)
    if c.edge is None:
        return
    single = [rc.counts([g], c.kind) for g in graphs]
    big = max(single, key=lambda k: rc.lds_bytes(k, 0))
    if c.edge == "A":
        got, step = rc.lds_bytes(big, 0), (4,)
        assert e["form"] == (0 if c.side == "fit" else 1)
    elif c.edge == "B":
        got, step = rc.lds_bytes(big, 1), (2, 4)
        assert (e["form"], e["train_form"]) == ((1, 1) if c.side == "fit" else (2, 2))
    elif c.edge == "C":
        assert big.U == (267 if c.side == "fit" else 268)
        assert rc.lds_bytes(big, 2) == (147256 if c.side == "fit" else 147804)
        assert e["active"] == int(c.side == "fit") and e.get("form", 2) == 2
        return
    else:
        assert all(k == single[0] for k in single)
        got, step = rc.lds_bytes(big, 0), (4,)
        assert e["form"] == 0 and e["graphs_per_workgroup"] == (2 if c.side == "fit" else 1)
        assert e["workgroups"] == ((len(graphs) + 1) // 2 if c.side == "fit" else len(graphs))
    assert e["active"] == 1
    assert got - rc.EXACT[c.edge] in ((0,) if c.side == "fit" else step), got


def test_every_edge_has_both_sides():
    sides = {(c.edge, c.side) for c in rc.CASES.values() if c.edge}
    assert sides == {(e, s) for e in "ABCD" for s in ("fit", "over")}
    exp = {n: rc.case_expected(n) for n in list(rc.CASES) + list(rc.ROWS16)}
    assert {e.get("form") for e in exp.values()} == {0, 1, 2, None}
    assert {(e["form"], e["graphs_per_workgroup"]) for e in exp.values() if e["active"]} >= {(0, 1), (0, 2), (1, 1), (1, 2), (2, 1)}
    # the named entries that are neither "fit" nor "over"
    assert exp["d_group_pg"]["form"] == 1 and exp["d_group_pg"]["workgroups"] == 1
    assert exp["d_group_268"] == {"active": 0} and exp["c_fallback"] == {"active": 0}
    assert exp["d_16bit_fit"]["active"] == 1 and exp["d_16bit_fit"]["graphs_per_workgroup"] == 2
    assert exp["d_16bit_over"] == {"active": 0}
    assert sum(g["num_path"] for g in rc.case_inputs("d_16bit_fit")[4]) == 65535
    # Q-size: the nodes' union rows start inside a tile
    for n in ("e_a_fit", "e_b_fit"):
        assert rc.case_inputs(n)[4][0]["num_link"] % 16 != 0
    # B's variants: link 0's in-degree on the segmented-sum switch, an idle link in a tile's last slot
    for hot in (63, 64, 65):
        (g,) = rc.case_inputs("b_over_hot%d" % hot)[4]
        assert np.bincount(g["src_adj_links_paths"])[0] == hot
    (g,) = rc.case_inputs("b_idle_last")[4]
    assert g["num_link"] % 16 == 0 and np.bincount(g["src_adj_links_paths"], minlength=g["num_link"])[-1] == 0
    # F: the grouped shape entries have a graph boundary inside a union-row tile, and lower at 2 and 3
    for n in rc.GROUPED:
        graphs = rc.case_inputs(n)[4]
        assert len(graphs) >= 2 and (n == "b16_16" or any(g["num_link"] % 16 for g in graphs[:-1]))   # (b16_16: on the edge)
        for k in (2, 3):
            e = rc.case_expected(n, group=k)
            assert e["active"] == 1 and e["graphs_per_workgroup"] == k and e["workgroups"] == -(-len(graphs) // k)


def test_tile_limit_is_behind_the_byte_limit():
    """kResidentMaxTiles (32 union-row tiles of one workgroup) cannot be reached: 33 tiles take at least
    16 * 31 + 2 = 498 union rows (two entities, each with a one-row last tile), and the CSR-global form,
    the smallest, already stops at 267."""
    fits = [U for U in range(1, 1000) if rc.lds_bytes(rc.Counts(U, 0, 0, 0, 0), 2) <= rc.LIMIT]
    assert fits == list(range(1, 268))
    fewest = min(a + b for a in range(520) for b in range(520) if (a + 15) // 16 + (b + 15) // 16 > rc.MAX_TILES)
    assert fewest == 498 > fits[-1]


@pytest.mark.parametrize("name", SMALL + ["d_16bit_fit"])
def test_oracle_is_well_conditioned(name):
    ref = rc.reference(name)
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() < 1.0
    assert ref.size == sum(g["num_path"] for g in rc.case_inputs(name)[4])
    if rc.case(name).grads:
        rc.grad_reference(name)   # asserts well_conditioned
