"""ign_batch_set_edge_params / ign_batch_enable_edge_param_gradients / ign_batch_edge_param_gradients
without a GPU: the symbols and their bindings, the ABI version they were added under, the refusals that
come before any device call, and the Python side's name and shape validation."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from ignnition_amd import _lib, model_examples, workloads
from ignnition_amd.engine import Batch, MPPlan, SplitBatch, edge_param_rows, edge_param_sources
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import edge_param_cases as ec

SOURCE_CALLS = ["ign_batch_set_edge_params", "ign_batch_edge_param_gradients"]
NEW = SOURCE_CALLS + ["ign_batch_enable_edge_param_gradients"]


def test_symbols_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "ignmp.h")).read()
    for name in SOURCE_CALLS:
        assert re.search(r"\bint\s+%s\(ign_plan\* plan, ign_batch\* batch, int32_t mp, int32_t source," % name, header), name
        assert getattr(_lib.lib, name).argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    assert re.search(r"\bint\s+ign_batch_enable_edge_param_gradients\(ign_plan\* plan, ign_batch\* batch\);", header)
    assert _lib.lib.ign_batch_enable_edge_param_gradients.argtypes == [C.c_void_p, C.c_void_p]
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib, name).restype is C.c_int
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)


def test_abi_version_stays_13():
    assert _lib.lib.ign_abi_version() == 13 == _lib.ABI_VERSION


def test_null_arguments_are_refused_before_any_device_call():
    for name in SOURCE_CALLS:
        assert getattr(_lib.lib, name)(None, None, 0, 0, None) == -1   # IGN_ERR_INVALID
        assert b"null argument" in _lib.lib.ign_last_error()
    assert _lib.lib.ign_batch_enable_edge_param_gradients(None, None) == -1
    assert b"null argument" in _lib.lib.ign_last_error()


def test_python_surface():
    for cls, names in ((Batch, ("set_edge_params", "edge_param_gradients", "enable_edge_param_gradients")),
                       (SplitBatch, ("set_edge_params", "edge_param_gradients")), (ComnetModel, ("sensitivities",))):
        for n in names:
            assert callable(getattr(cls, n))
    assert "params_<adj>" in ComnetModel.sensitivities.__doc__
    assert "edge_param_gradients" in Batch.enable_training.__code__.co_varnames


def _plan(name):
    desc, dims = ec.case_inputs(name)[:2]
    return MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))


def test_sources_of_an_adjacency():
    assert edge_param_sources(_plan("sum_p3_last"), "adj_paths_links") == (3, [(1, 0, 1)])
    assert edge_param_sources(_plan("ordered_mixed"), "adj_links_paths") == (2, [(0, 0, 0)])
    assert edge_param_sources(_plan("two_mps_p2"), "adj_paths_links") == (2, [(1, 0, 1), (2, 0, 1)])
    for name in ec.CASES:
        assert ec.slice_columns(_plan(name), ec.ADJ[name]) == ec.COLUMNS[name], name


def test_an_adjacency_nothing_reads_is_a_value_error():
    with pytest.raises(ValueError, match=r"no message network reads the edge parameters of adjacency 'adj_links_paths' "
                                         r"\(read: \['adj_paths_links'\]\)"):
        edge_param_sources(_plan("sum_p3_last"), "adj_links_paths")
    with pytest.raises(ValueError, match="adjacency 'nope'"):
        edge_param_sources(_plan("sum_p3_last"), "nope")
    # a message network that reads states only; and no message network at all
    desc = model_examples.routenet_message_net(inputs=("hs_source", "hs_dest"), iterations=2)
    _, dims, _ = workloads.model("routenet")
    with pytest.raises(ValueError, match=r"\(read: \[\]\)"):
        edge_param_sources(MPPlan.from_model_info(Model_information(desc, dims)), "adj_paths_links")
    with pytest.raises(ValueError, match=r"\(read: \[\]\)"):
        edge_param_sources(MPPlan.from_model_info(Model_information(model_examples.routenet(), dims)), "adj_paths_links")


def test_rows_are_taken_in_edge_order():
    a = np.arange(15, dtype=np.float64).reshape(5, 3)
    got = edge_param_rows(5, 3, a)
    assert got.dtype == np.float32 and got.shape == (5, 3) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, a.astype(np.float32))
    assert np.array_equal(edge_param_rows(5, 3, a.reshape(-1)), got)
    assert np.array_equal(edge_param_rows(4, 1, [1, 2, 3, 4]), np.array([[1], [2], [3], [4]], np.float32))
    assert edge_param_rows(0, 2, np.zeros((0, 2))).shape == (0, 2)


@pytest.mark.parametrize("values,text", [
    (np.zeros((4, 3)), "set_edge_params: values have shape (4, 3), the batch needs 5 rows of width 3"),
    (np.zeros((5, 2)), "values have shape (5, 2)"),
    (np.zeros((3, 5)), "values have shape (3, 5)"),      # the right count in the wrong shape
    (np.zeros((5, 3, 1)), "values have shape (5, 3, 1)"),
    (np.zeros(14), "values have shape (14,)"),
])
def test_wrong_shapes_are_value_errors(values, text):
    with pytest.raises(ValueError) as e:
        edge_param_rows(5, 3, values)
    assert text in str(e.value)


class _NoDevice:
    """A Batch as far as the validation reads it: any call into the library would fail on the handles."""
    handle = None

    def __init__(self, plan, edges):
        self.engine = type("E", (), {"plan": plan, "handle": None, "device": 0})()
        self.graph_edges = np.asarray(edges, np.int64)

    _edge_sources = Batch._edge_sources
    set_edge_params = Batch.set_edge_params
    edge_param_gradients = Batch.edge_param_gradients


def test_batch_validation_raises_before_any_device_call():
    b = _NoDevice(_plan("sum_p3_last"), [[7, 5], [7, 4]])   # [graphs, adjacency slots]: 9 edges of slot 1
    assert b._edge_sources("adj_paths_links") == (9, 3, [(1, 0)])
    with pytest.raises(ValueError, match="the batch needs 9 rows of width 3"):
        b.set_edge_params("adj_paths_links", np.zeros((10, 3), np.float32))
    with pytest.raises(ValueError, match="no message network reads"):
        b.set_edge_params("adj_links_paths", np.zeros((14, 3), np.float32))
    with pytest.raises(ValueError, match="no message network reads"):
        b.edge_param_gradients("adj_links_paths")
    with pytest.raises(ValueError, match="out must be a CUDA tensor"):
        b.edge_param_gradients("adj_paths_links", out=np.zeros((9, 3), np.float32))
