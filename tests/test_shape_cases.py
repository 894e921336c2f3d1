"""The routing-level graph builder and its table (tests/shape_cases.py) on the CPU: every entry builds with
the counts it names, the generator emits a built graph from the sample that restates it, and the two
float64 restatements agree on every entry (1e-10, as tests/test_oracle.py holds them on its inputs)."""
import numpy as np
import pytest

from ignnition_amd import workloads
from ignnition_amd.json_operations import Model_information
from oracle.packed_forward import PackedOracle
from tests import shape_cases as sc

ALL = sorted(sc.SHAPES)


@pytest.mark.parametrize("name", ALL)
def test_entry_builds_with_the_requested_counts(name):
    s = sc.SHAPES[name]
    assert s.hidden in (16, 32, 64) and s.kind in ("routenet", "qsize")
    _, _, _, plan, graphs, labels, _ = sc.case_inputs(name)
    assert plan.hidden == [s.hidden] * len(plan.entities) and plan.iterations == sc.ITERATIONS
    for spec, g, y in zip(s.graphs, graphs, labels):
        a = dict(spec)
        lens = np.asarray(a["lens"])
        P, L = a["P"], a["L"] + a.get("idle_links", 0)
        assert P <= 257 and L <= 35
        assert (g["num_path"], g["num_link"], y.size) == (P, L, P)
        assert g["traffic"].shape == (P,) and g["link_capacity"].shape == (L,)
        assert g["traffic"].dtype == np.float32 and np.abs(g["traffic"]).max() <= 1
        np.testing.assert_array_equal(np.bincount(g["dst_adj_links_paths"], minlength=P), lens)
        deg = np.bincount(g["src_adj_links_paths"], minlength=L)
        np.testing.assert_array_equal(deg, np.bincount(g["dst_adj_paths_links"], minlength=L))
        assert np.all(deg[a["L"]:] == 0)
        if "hot" in a:
            assert deg[0] == a["hot"]
        for p in range(P):   # distinct links at positions 0 .. len - 1
            on = np.asarray(g["dst_adj_links_paths"]) == p
            assert sorted(np.asarray(g["seq_link_path"])[on]) == list(range(lens[p]))
            assert np.unique(np.asarray(g["src_adj_links_paths"])[on]).size == lens[p]
        if s.kind == "qsize":
            assert g["num_node"] == a["N"] and g["queue_sizes"].shape == (a["N"],)
            ndeg = np.bincount(g["src_adj_nodes_paths"], minlength=a["N"])
            np.testing.assert_array_equal(np.bincount(g["dst_adj_nodes_paths"], minlength=P), lens)
            if "hot_node" in a:
                assert ndeg[0] == a["hot_node"]
            assert len(g["indices_link_to_path"]) == len(g["indices_node_to_path"]) == lens.max()


def test_table_covers_the_edges():
    """The row counts and in-degrees the table is there for, read back from the built graphs."""
    one = {n: sc.case_inputs(n)[4] for n, s in sc.SHAPES.items() if s.hidden == 32 and not s.env and s.kind == "routenet"}
    paths = {g["num_path"] for gs in one.values() if len(gs) == 1 for g in gs}
    links = {g["num_link"] for gs in one.values() if len(gs) == 1 for g in gs}
    deg0 = {int(np.bincount(g["src_adj_links_paths"], minlength=1)[0]) for gs in one.values() for g in gs}
    assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257} <= paths
    assert {1, 2, 15, 16, 17, 33} <= links
    assert {0, 1, 63, 64, 65} <= deg0
    assert sorted(sum(g["num_path"] for g in gs) for gs in one.values() if len(gs) > 1) == [16, 32, 54, 64]
    nodes = {g["num_node"] for n, s in sc.SHAPES.items() if s.kind == "qsize" for g in sc.case_inputs(n)[4]}
    assert {1, 16, 17} <= nodes
    assert int(np.bincount(sc.case_inputs("qs_node64")[4][0]["src_adj_nodes_paths"])[0]) == 64
    assert sc.SHAPES["l15_idle"].graphs and sc.case_inputs("l15_idle")[4][0]["num_link"] == 16
    assert sc.case_inputs("l16_idle")[4][0]["num_link"] == 17


@pytest.mark.parametrize("name", ["p17", "deg65", "l16_idle", "long17_mid", "qs_n17", "qs_node64"])
def test_generator_emits_the_built_arrays(name):
    """generator.sample_to_data (through workloads.graph_inputs) on the sample that restates a built graph
    gives that graph: every index list, the counts, the interleave indices and the features."""
    s = sc.SHAPES[name]
    desc, dims = sc.model(s.kind, s.hidden)
    mi = Model_information(desc, dims)
    built = sc.case_inputs(name)[4][0]
    sample = (sc.qsize_sample_of if s.kind == "qsize" else sc.routenet_sample_of)(built)
    (got,), _ = workloads.graph_inputs(mi, [sample])
    assert set(got) == set(built)
    for k, v in built.items():
        if np.asarray(v).dtype.kind == "f":
            np.testing.assert_array_equal(np.asarray(got[k], np.float32), v, err_msg=k)
        else:
            assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k


@pytest.mark.parametrize("name", ALL)
def test_dense_and_packed_restatements_agree(name):
    desc, dims, _, _, graphs, _, prm = sc.case_inputs(name)
    ref = sc.reference(name)
    assert np.all(np.isfinite(ref)) and ref.size == sum(g["num_path"] for g in graphs)
    np.testing.assert_allclose(ref, PackedOracle(desc, dims, prm).forward(graphs), rtol=1e-10, atol=1e-12)
