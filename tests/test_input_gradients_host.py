"""ign_batch_set_features / ign_batch_feature_gradients without a GPU: the symbols and their bindings,
the ABI version they were added under, and the host assembly of ``Batch.set_features``' rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ignnition_amd import _lib
from ignnition_amd.engine import Batch, SplitBatch, feature_rows
from ignnition_amd.generate_model import ComnetModel

NEW = ["ign_batch_set_features", "ign_batch_feature_gradients"]


def test_symbols_exported_and_bound():
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "ignmp.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\(ign_plan\* plan, ign_batch\* batch, int32_t entity," % name, header), name
        assert name in _lib.SYMBOLS
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int
        assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)


def test_abi_version_stays_13():
    assert _lib.lib.ign_abi_version() == 13 == _lib.ABI_VERSION


def test_null_arguments_are_refused_before_any_device_call():
    for name in NEW:
        assert getattr(_lib.lib, name)(None, None, 0, None) == -1   # IGN_ERR_INVALID
        assert b"null argument" in _lib.lib.ign_last_error()


def test_python_surface():
    for cls, names in ((Batch, ("set_features", "feature_gradients")), (SplitBatch, ("set_features",)),
                       (ComnetModel, ("sensitivities",))):
        for n in names:
            assert callable(getattr(cls, n))
    assert "normalised" in ComnetModel.sensitivities.__doc__


FEATS = [("link_capacity", 3), ("link_load", 2), ("up", 1)]


def test_dict_is_assembled_in_plan_order():
    rng = np.random.default_rng(0)
    cap, load, up = rng.normal(size=(5, 3)), rng.normal(size=(5, 2)), rng.normal(size=5)
    # given out of order; size-1 as [rows]; a wide one flat, and as float64: the rows are float32
    got = feature_rows(FEATS, 5, {"up": up, "link_load": load.reshape(-1), "link_capacity": cap})
    assert got.dtype == np.float32 and got.shape == (5, 6) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, np.concatenate([cap, load, up[:, None]], 1).astype(np.float32))
    assert np.array_equal(feature_rows(FEATS, 5, {"up": up[:, None], "link_load": load, "link_capacity": cap}), got)


def test_one_array_is_taken_as_rows():
    a = np.arange(30, dtype=np.float64).reshape(5, 6)
    assert np.array_equal(feature_rows(FEATS, 5, a), a.astype(np.float32))
    assert np.array_equal(feature_rows(FEATS, 5, a.reshape(-1)), a.astype(np.float32))
    assert np.array_equal(feature_rows([("traffic", 1)], 4, [1, 2, 3, 4]), np.array([[1], [2], [3], [4]], np.float32))
    src = np.zeros((5, 6), np.float32)
    out = feature_rows(FEATS, 5, src)
    assert out.shape == (5, 6)


@pytest.mark.parametrize("values,text", [
    ({"link_capacity": np.zeros((5, 3)), "link_load": np.zeros((5, 2))}, "missing feature(s) ['up']"),
    ({"link_capacity": np.zeros((5, 3)), "link_load": np.zeros((5, 2)), "up": np.zeros(5), "traffic": np.zeros(5)},
     "unknown feature(s) ['traffic']"),
    ({"link_capacity": np.zeros((4, 3)), "link_load": np.zeros((5, 2)), "up": np.zeros(5)},
     "feature link_capacity has shape (4, 3), the batch needs 5 rows of width 3"),
    ({"link_capacity": np.zeros((3, 5)), "link_load": np.zeros((5, 2)), "up": np.zeros(5)},
     "feature link_capacity has shape (3, 5)"),     # the right count in the wrong shape
    ({"link_capacity": np.zeros((5, 3)), "link_load": np.zeros((5, 2)), "up": np.zeros((5, 1, 1))},
     "feature up has shape (5, 1, 1)"),
    (np.zeros((4, 6)), "values have shape (4, 6), the batch needs 5 rows of width 6"),
    (np.zeros((5, 5)), "values have shape (5, 5)"),
    (np.zeros((6, 5)), "values have shape (6, 5)"),
])
def test_wrong_columns_are_value_errors(values, text):
    with pytest.raises(ValueError) as e:
        feature_rows(FEATS, 5, values)
    assert text in str(e.value)


def test_an_entity_without_features_is_a_value_error():
    with pytest.raises(ValueError, match="no features"):
        feature_rows([], 5, np.zeros((5, 0)))
