"""The table of tests/gru_shape_cases.py on the CPU: the conditions tests/test_gpu_gru_shapes.py relies on,
shown on the float64 reference alone.  Every entry's loss is well conditioned (shape_cases.well_conditioned),
its predictions are not constant, every gradient tensor of the autograd oracle is finite and non-zero and
there is one per parameter, 4 x the float32 run's error stays below test_gpu_parity's TOL (so no entry
widens the GPU tests' bound), and the property the entry is named for is read back from its built graphs.
The table covers every (option set, kind of edge) pair it promises."""
import numpy as np
import pytest

from tests import gru_shape_cases as gs
from tests import shape_cases as sc

TOL = 1e-4   # tests/test_gpu_parity.py's TOL (that module needs no GPU to import, but is marked gpu as a whole)
ALL = sorted(gs.CASES)


def _one(name):
    graphs = gs.case_inputs(name)[4]
    assert len(graphs) == 1
    return graphs[0]


def _link_degrees(g):
    return np.bincount(np.asarray(g["dst_adj_paths_links"], np.int64), minlength=int(g["num_link"]))


def _lengths(g):
    return np.bincount(np.asarray(g["dst_adj_links_paths"], np.int64), minlength=int(g["num_path"]))


def test_tol_is_the_parity_tests():
    from tests.test_gpu_parity import TOL as parity_tol
    assert TOL == parity_tol


@pytest.mark.parametrize("name", ALL)
def test_reference_meets_the_gpu_tests_conditions(name):
    s, options, kw = gs.CASES[name]
    desc, dims, _, plan, graphs, labels, prm = gs.case_inputs(name)
    assert plan.iterations == gs.T
    assert set(plan.hidden) == ({16, 32} if "widths" in kw else {s.hidden})
    pred, states = gs.reference(name)
    rows = sum(int(g["num_path"]) for g in graphs)
    assert pred.shape == (rows,) and np.isfinite(pred).all()
    for e, st in states.items():
        assert np.isfinite(st).all() and st.shape[0] == sum(int(g["num_" + e]) for g in graphs)
    sc.well_conditioned(labels, pred)
    assert rows == 1 or np.ptp(pred) > 1e-3, "the oracle's predictions are constant"
    f32 = gs.float32_error(name)
    print("%s: float32 numpy run vs float64: max scaled error %.3g (x4 = %.3g)" % (name, f32, 4 * f32))
    assert 4 * f32 <= TOL
    loss, _, grads, o_pred = gs.autograd(name)
    np.testing.assert_allclose(o_pred, pred, rtol=1e-10, atol=1e-12)   # the two restatements agree
    assert np.isfinite(loss)
    assert set(grads) == set(prm) == {n for n, _ in plan.param_specs()}
    biases = [k for k in prm if k.endswith("_update/bias")]
    if s.kind == "qsize":   # the path cell alone takes the options
        assert ("path_update/bias" in prm) == options.get("use_bias", True) and len(biases) >= 2
    else:
        assert bool(biases) == options.get("use_bias", True)
    for k, g in grads.items():
        assert g.shape == prm[k].shape and np.isfinite(g).all() and np.linalg.norm(g) > 0, k


_ROWS = {"p1": 1, "p16": 16, "p17": 17, "p33": 33, "p63": 63, "p64": 64, "p65": 65, "p129": 129, "p257": 257,
         "h16_p17": 17, "h64_p17": 17, "len_all_1": 24, "len_all_L": 10}
_LINKS = {"l1": 1, "l16": 16, "l17": 17, "l33": 33, "l15_idle": 16, "l16_idle": 17, "h64_l191": 191, "h64_l192": 192,
          "h64_l193": 193}
_DEG0 = {"deg0": 0, "deg1": 1, "deg63": 63, "deg64": 64, "deg65": 65, "deg64_win": 64, "deg65_win": 65,
         "h16_deg64": 64, "h64_deg64": 64}


@pytest.mark.parametrize("name", ALL)
def test_entry_has_the_property_it_is_named_for(name):
    shape = name.split("/")[0]
    s = gs.CASES[name][0]
    graphs = gs.case_inputs(name)[4]
    known = 0
    if shape in _ROWS:
        known += 1
        assert _one(name)["num_path"] == _ROWS[shape]
    if shape in _LINKS:
        known += 1
        g = _one(name)
        assert g["num_link"] == _LINKS[shape]
        if shape.endswith("_idle"):
            assert _link_degrees(g)[-1] == 0 and np.all(_link_degrees(g)[:-1] > 0)
        if shape.startswith("h64_l"):
            assert s.hidden == 64 and np.all(_lengths(g) == 2)
    if shape in _DEG0:
        known += 1
        assert _link_degrees(_one(name))[0] == _DEG0[shape]
        assert (("IGN_SUM_WINDOW", "1") in s.env) == shape.endswith("_win")
    if shape.startswith("long"):
        known += 1
        lens = _lengths(_one(name))
        at = {"first": 0, "mid": 8, "last": 19}[shape.split("_")[1]]
        assert lens.max() == lens[at] == int(shape[4:6]) and np.all(np.delete(lens, at) == 1)
    if shape == "len_all_1":
        assert np.all(_lengths(_one(name)) == 1)
    if shape == "len_all_L":
        assert np.all(_lengths(_one(name)) == _one(name)["num_link"])
    if shape == "b16_16":
        known += 1
        assert [g["num_path"] for g in graphs] == [16, 16]
    if shape == "b_p1_between":
        known += 1
        assert [g["num_path"] for g in graphs] == [20, 1, 33]
    if shape.startswith("qs_"):
        known += 1
        g = _one(name)
        ndeg = np.bincount(np.asarray(g["dst_adj_paths_nodes"], np.int64), minlength=int(g["num_node"]))
        assert g["num_node"] == {"qs_n1": 1, "qs_n17": 17, "qs_node64": 4}[shape]
        assert shape != "qs_node64" or ndeg[0] == 64
    assert known == 1, "no property is read back for " + name


def test_pre_summed_entries_have_a_row_of_64_messages():
    """The entries whose training forward must take the pre-summed route: an in-degree >= 64 (or the
    windowed sum) on a plain sum MP of a plan with an option cell."""
    for name in ("deg64/V1", "deg65/V1", "deg65/ALL_FOUR", "deg64_win/V1", "deg65_win/V1", "h16_deg64/V1",
                 "h64_deg64/V1", "qs_node64/V1", "deg64/V1/l16_p32", "deg65/V1/attention"):
        assert gs.max_in_degree(name) >= 64, name
    for name in ("deg63/V1", "deg1/V1", "l33/V1", "h64_l193/V1"):
        assert gs.max_in_degree(name) < 64, name


def test_table_covers_every_promised_pair():
    shapes = lambda option, tag=None: {n.split("/")[0] for n in gs.CASES
                                       if n.split("/")[1] == option and (n.split("/")[2:] or [None])[0] == tag}
    every = set(gs.ORDERED + gs.LENGTHS + gs.SUM_ROWS + gs.DEGREES + gs.WIDTHS + gs.QSIZE) | set(gs.H64_ROWS)
    assert shapes("V1") == every
    assert {"p1", "p16", "p17", "p33", "p63", "p64", "p65", "p129", "p257", "len_all_1", "len_all_L", "long16_first",
            "long16_mid", "long16_last", "long17_mid", "long33_first", "long33_mid", "long33_last", "b16_16",
            "b_p1_between", "l1", "l16", "l17", "l33", "l15_idle", "l16_idle", "deg0", "deg1", "deg63", "deg64",
            "deg65", "deg64_win", "deg65_win", "h16_p17", "h16_deg64", "h64_p17", "h64_deg64", "h64_l191",
            "h64_l192", "h64_l193", "qs_n1", "qs_n17", "qs_node64"} == every
    assert shapes("V1", "l16_p32") == {"l17", "deg64"}
    assert shapes("V1", "attention") == shapes("V1", "convolution") == {"l17", "deg1", "deg65"}
    for option in ("ALL_FOUR", "HS_NO_BIAS", "RELU"):
        kinds = {gs.KIND[n] for n in gs.CASES if n.split("/")[1] == option}
        assert kinds == set(gs.SPREAD_KINDS), (option, kinds)
    assert "p257/RELU" not in gs.CASES
    assert set(gs.KIND) == set(gs.CASES)
    for name in gs.TS_CASES + gs.ADAM_CASES + gs.FEATURE_GRAD_CASES:
        assert name in gs.CASES
    # the option sets are gru_cases', and the kernels' template arguments are the promised ones
    assert gs.OPTIONS["V1"] == {"reset_after": False} and gs.OPTIONS["HS_NO_BIAS"].get("reset_after", True)
    for name, (s, _, kw) in gs.CASES.items():
        plan = gs.case_inputs(name)[3]
        if "widths" in kw:
            assert dict(zip(plan.entities, plan.hidden)) == {"link": 16, "path": 32}
        assert [m["aggregation"] for m in _sum_mps(gs.case_inputs(name)[0])] == \
            [kw.get("aggregation", {"type": "sum"})["type"]] * (2 if s.kind == "qsize" else 1)


def _sum_mps(desc):
    out = []
    for stage in desc["message_passing"]["stages"]:
        for mp in stage["stage_mp"]:
            if mp["destination_entity"] != "path":
                out.append({"aggregation": mp["aggregation"]["type"]})
    return out
