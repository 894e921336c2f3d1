"""HIP engine vs the oracle, through the C ABI (MI355X only).

Tolerance (fp32 engine vs float64 oracle, after T=8 iterations and the readout):
  |engine - oracle| <= 1e-4 * max(1, |oracle|)         
Hidden states are checked with the same bound.  Indices are integer and exact by
construction (the engine consumes the generator's arrays unchanged).
"""
import copy

import numpy as np
import pytest

from ignnition_amd import _lib, model_examples, synthetic, workloads
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from oracle import cpu_oracle
from oracle.dense_forward import DenseOracle

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _ieee_tol(plan, graphs, prm, ref):
    """The tolerance of a case whose float32 arithmetic itself may exceed TOL: 1.5x the maximum scaled
    error of the IEEE float32 build of the C++ restatement (oracle/cpu_forward.cpp, libm expf / tanhf,
    no reassociation) on the SAME graphs and parameters -- test_gpu_fullsize.py's rule for the maximum
    -- and TOL wherever that yardstick lies below TOL / 1.5."""
    ieee = cpu_oracle.cpu_forward(plan, graphs, prm, 0, ieee=True)
    exp = np.asarray(ref, np.float64).reshape(-1)
    yard = float((np.abs(ieee - exp) / np.maximum(1.0, np.abs(exp))).max())
    print("IEEE float32 yardstick: max scaled error %.3g -> tolerance %.3g" % (yard, max(TOL, 1.5 * yard)))
    return max(TOL, 1.5 * yard)


def _close(got, exp, tol=TOL):
    got = np.asarray(got, np.float64).reshape(-1)
    exp = np.asarray(exp, np.float64).reshape(-1)
    err = np.abs(got - exp) / np.maximum(1.0, np.abs(exp))
    assert got.shape == exp.shape
    assert np.all(np.isfinite(got))
    assert err.max() <= tol, "max scaled error %.3g at %d" % (err.max(), int(err.argmax()))


def _run(desc, dims, graphs, seed=0, bias=0.05):
    mi = Model_information(copy.deepcopy(desc), dims)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(seed, bias_scale=bias)
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    out = b.forward()
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    return out, ref, b, prm


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


@pytest.mark.parametrize("kind,topo,n", [("routenet", "nsfnet", 1), ("routenet", "nsfnet", 3),
                                         ("routenet", "geant2", 2), ("qsize", "nsfnet", 2)])
def test_forward_matches_oracle(kind, topo, n):
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs(kind, topo, n)
    out, ref, b, _ = _run(desc, dims, graphs)
    _close(out, ref)
    assert b.edges_per_forward == workloads.edges_per_forward(mi, graphs)


@pytest.mark.parametrize("hidden", [16, 32, 64])
def test_hidden_sizes(hidden):
    desc = model_examples.routenet(hidden=hidden, iterations=3)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 11)])
    out, ref, _, _ = _run(desc, dims, graphs, seed=2, bias=0.3)
    _close(out, ref)


def test_zero_gru_known_answer_on_gpu():
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "nsfnet", 1)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(0)
    for k in prm:
        if "_update/" in k:
            prm[k] = np.zeros_like(prm[k])
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    b.forward()
    g = graphs[0]
    L = np.bincount(np.asarray(g["dst_adj_links_paths"]), minlength=g["num_path"])
    path = b.state("path")
    np.testing.assert_allclose(path[:, 0], np.asarray(g["traffic"]) * 0.5 ** (8 * L), rtol=1e-6, atol=1e-30)
    assert np.all(path[:, 1:] == 0)


def test_interleave_holes_and_dropped_positions():
    from tests.test_oracle import QS_DIMS, holes_input
    desc = model_examples.qsize(hidden=16, iterations=3)
    out, ref, _, _ = _run(desc, QS_DIMS, [holes_input(), holes_input()], seed=7, bias=0.3)
    _close(out, ref)


def test_duplicate_positions_accumulate():
    """scatter_nd adds messages that share (dst, seq) (GM:490): two links at position 0 of
    path 0, a hole at position 1, one link at position 2 (final_len 3 = Lmax 3)."""
    desc = model_examples.routenet(hidden=16, iterations=2)
    dims = {"link_capacity": 1, "traffic": 1, "adj_links_paths": 0, "adj_paths_links": 0}
    x = {"link_capacity": [0.5, -0.3, 0.8], "traffic": [0.2, -0.4],
         "src_adj_links_paths": [0, 1, 2, 2], "dst_adj_links_paths": [0, 0, 0, 1], "seq_link_path": [0, 0, 2, 0],
         "src_adj_paths_links": [0, 1, 0], "dst_adj_paths_links": [0, 1, 2], "seq_path_link": [0, 0, 0],
         "num_link": 3, "num_path": 2}
    out, ref, _, _ = _run(desc, dims, [x], seed=3, bias=0.2)
    _close(out, ref)


def test_multi_source_ordered_slots_after_global_lmax():
    """Two sources with 'ordered': source 2's slots start after source 1's Lmax (GM:533),
    leaving holes for destinations with fewer source-1 messages."""
    desc = model_examples.qsize(hidden=16, iterations=2)
    desc["message_passing"]["stages"][0]["stage_mp"][0]["aggregation"] = {"type": "ordered"}
    from tests.test_oracle import QS_DIMS, holes_input
    x = holes_input()
    del x["indices_link_to_path"], x["indices_node_to_path"]
    out, ref, _, _ = _run(desc, QS_DIMS, [x], seed=9, bias=0.3)
    _close(out, ref)


@pytest.mark.parametrize("aggr", ["interleave", "ordered"])
def test_narrow_sequence_mask_rejected(aggr):
    """max(final_len) < padded length in a graph: the reference's masked RNN reads its
    sequence_mask TensorList past the end and TF raises (AUX:785-790); the engine
    returns IGN_ERR_INVALID, the oracle raises.  The same graph next to a full-width one (the
    batch of the reference is per graph) still fails."""
    from tests.test_oracle import QS_DIMS, holes_input, narrow_mask_input
    desc = model_examples.qsize(hidden=16, iterations=2)
    x = narrow_mask_input()
    ok = holes_input()
    if aggr == "ordered":
        desc["message_passing"]["stages"][0]["stage_mp"][0]["aggregation"] = {"type": "ordered"}
        for g in (x, ok):
            del g["indices_link_to_path"], g["indices_node_to_path"]
    mi = Model_information(copy.deepcopy(desc), QS_DIMS)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(0))
    for graphs in ([x], [ok, x]):
        with pytest.raises(_lib.EngineError, match="sequence_mask") as ei:
            Batch(eng, graphs)
        assert ei.value.code == -1
    Batch(eng, [ok]).forward()


def test_final_len_beyond_padding_rejected():
    """Duplicates that make final_len exceed max(seq)+1: TF's gather_nd fails (AUX:793-795)."""
    desc = model_examples.routenet(hidden=16, iterations=2)
    dims = {"link_capacity": 1, "traffic": 1, "adj_links_paths": 0, "adj_paths_links": 0}
    x = {"link_capacity": [0.5, -0.3, 0.8], "traffic": [0.2, -0.4],
         "src_adj_links_paths": [0, 1, 2, 2], "dst_adj_links_paths": [0, 0, 0, 1], "seq_link_path": [0, 0, 1, 0],
         "src_adj_paths_links": [0, 1, 0], "dst_adj_paths_links": [0, 1, 2], "seq_path_link": [0, 0, 0],
         "num_link": 3, "num_path": 2}
    mi = Model_information(copy.deepcopy(desc), dims)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(0))
    with pytest.raises(_lib.EngineError, match="gather_nd"):
        Batch(eng, [x])


def test_error_paths_match_reference():
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "nsfnet", 1)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(0))
    g = dict(graphs[0])
    keep = np.asarray(g["dst_adj_links_paths"]) != 0
    for k in ("src_adj_links_paths", "dst_adj_links_paths", "seq_link_path"):
        g[k] = np.asarray(g[k])[keep]
    with pytest.raises(_lib.EngineError) as ei:
        Batch(eng, [g])
    assert ei.value.code == -1 and "no message" in str(ei.value)
    g = dict(graphs[0])
    g["src_adj_paths_links"] = np.asarray(g["src_adj_paths_links"]).copy()
    g["src_adj_paths_links"][3] = 10 ** 6
    with pytest.raises(_lib.EngineError):
        Batch(eng, [g])


def test_ragged_interleave_rejected(gen_fixtures):
    from tests.test_oracle import QS_DIMS
    case = [c for c in gen_fixtures if c["name"] == "interleave_ragged"][0]
    x = dict(case["expected"][0]["data"])
    mi = Model_information(model_examples.qsize(hidden=16), QS_DIMS)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(0))
    with pytest.raises(_lib.EngineError, match="different lengths"):
        Batch(eng, [x])


def test_batch_equals_per_graph():
    """Disjoint-union batching == the reference's per-graph loop + concat (GM:712-724)."""
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("qsize", "nsfnet", 3)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(4, bias_scale=0.1))
    whole = Batch(eng, graphs).forward().reshape(-1)
    parts = np.concatenate([Batch(eng, [g]).forward().reshape(-1) for g in graphs])
    np.testing.assert_array_equal(whole, parts)


def test_large_batch_properties():
    """64 x synth50-size batch: finite, deterministic, and graph g of the batch equals the same
    graph run alone (size-independent property), plus a graph vs the oracle.  The full 512-graph
    batch is tests/test_gpu_fullsize.py::test_routenet_512_synth50_batch."""
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "synth50", 64)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(1, bias_scale=0.05)
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    o1 = b.forward().reshape(-1)
    o2 = b.forward().reshape(-1)
    np.testing.assert_array_equal(o1, o2)
    assert np.all(np.isfinite(o1))
    P = [int(g["num_path"]) for g in graphs]
    off = np.cumsum([0] + P)
    for gi in (0, 17, 63):
        alone = Batch(eng, [graphs[gi]]).forward().reshape(-1)
        np.testing.assert_array_equal(o1[off[gi]:off[gi + 1]], alone)
    ref = DenseOracle(desc, dims, prm).forward([graphs[5]])
    _close(o1[off[5]:off[6]], ref)


def test_synthetic_graph_h64_matches_oracle():
    """The 1M-node config's model (single entity, sum + 64-unit GRU, 3-layer readout) on a
    2 000-node instance of the same generator."""
    desc, dims, mi, graphs, _ = workloads.make_synthetic_inputs(n_nodes=2000, iterations=3, window=64)
    out, ref, b, _ = _run(desc, dims, graphs, seed=4, bias=0.1)
    _close(out, ref)
    assert b.edges_per_forward == 3 * len(graphs[0]["src_adj_nodes_nodes"])


def test_hip_graph_replay_matches_direct(monkeypatch):
    """The captured hipGraph replays the same launches: bitwise-equal predictions.  Timed
    forwards launch directly, and the per-kernel event timing covers every launch (the batched
    launches: the resident forward is off here, test_resident_forward_is_the_batched_forward)."""
    monkeypatch.setenv("IGN_RESIDENT", "0")
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "geant2", 3)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(1, bias_scale=0.1)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("IGN_HIP_GRAPH", mode)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        b = Batch(eng, graphs)
        first = b.forward()                      # graph captured here (mode 1)
        second = b.forward()                     # ... and replayed
        np.testing.assert_array_equal(first, second)
        eng.set_timing(True)
        timed = b.forward()
        b.forward()
        st = eng.stats()
        np.testing.assert_array_equal(first, timed)
        assert st["seq_gru"]["launches"] == 2 * plan.iterations
        assert st["sum_gru"]["launches"] == 2 * plan.iterations
        assert st["readout"]["launches"] == 2 and st["seq_gru"]["ms"] > 0
        outs[mode] = first
        b.close()
        eng.close()
    np.testing.assert_array_equal(outs["0"], outs["1"])


@pytest.mark.parametrize("hidden", [32, 64])
def test_ordered_update_f32_variant_matches_oracle(monkeypatch, hidden):
    """The f32-MFMA ordered update (IGN_SEQ_VARIANT=2, the split-bf16 default's reference form):
    deterministic, and within the parity tolerance of the oracle."""
    desc = model_examples.routenet(hidden=hidden, iterations=3)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("geant2", g) for g in range(3)])
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(3, bias_scale=0.2)
    monkeypatch.setenv("IGN_SEQ_VARIANT", "2")
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    out = b.forward().reshape(-1)
    np.testing.assert_array_equal(out, b.forward().reshape(-1))
    b.close()
    eng.close()
    _close(out, DenseOracle(desc, dims, prm).forward(graphs))


def _scaled_err(got, exp):
    got = np.asarray(got, np.float64).reshape(-1)
    exp = np.asarray(exp, np.float64).reshape(-1)
    return float((np.abs(got - exp) / np.maximum(1.0, np.abs(exp))).max())


@pytest.mark.parametrize("hidden", [32, 64])
def test_split_bf16_contractions_are_fp32_accurate(monkeypatch, hidden):
    """Ordered-update variant 4 and readout variant 2 form their contractions from exact 3-piece
    bf16 splits (6 piece products, fp32 accumulation); ordered-update variant 6 and readout
    variants 4 and 5 (the latter on 32x32x16 MFMAs) from scaled 2-piece fp16 splits (3 piece products).  Their error vs the
    float64 oracle stays at the level of the native f32-MFMA kernels (seq 2, readout 1): within
    4x of it (or 1e-6), far inside the 1e-4 parity tolerance."""
    desc = model_examples.routenet(hidden=hidden, iterations=8)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("geant2", g) for g in range(3)])
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(5, bias_scale=0.2)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    errs = {}
    for seq, ro in (("2", "1"), ("4", "1"), ("6", "1"), ("2", "2"), ("4", "2"), ("2", "4"), ("6", "4"), ("2", "5"),
                    ("6", "5")):
        monkeypatch.setenv("IGN_SEQ_VARIANT", seq)
        monkeypatch.setenv("IGN_READOUT_VARIANT", ro)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        b = Batch(eng, graphs)
        out = b.forward().reshape(-1)
        b.close()
        eng.close()
        _close(out, ref)
        errs[seq + "/" + ro] = _scaled_err(out, ref)
    print("max scaled error vs float64 oracle (seq/readout variant):", errs)
    for k, v in errs.items():
        assert v <= max(4 * errs["2/1"], 1e-6), errs


@pytest.mark.parametrize("hidden", [32, 64])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 3e4])
def test_split_fp16_scaling(monkeypatch, hidden, scale):
    """Ordered-update variant 6 scales the state by a power of two per 16-row tile (from the
    tile's max |h|, which the GRU never exceeds along the sequence) and U by one at pack time;
    readout variants 4 and 5 (16- and 32-row tiles) scale each row tile's layer-2 input from a bound on the layer-1
    activations (max |x| of the tile, W1's column norms, b1) and W2 at pack time.  So the fp16
    pieces neither overflow nor lose bits: path features of 1e-3, 1 and 3e4 (the path state
    starts as [traffic | 0], the readout reads the path states) stay within the f32-MFMA
    variants' error class vs the float64 oracle, and repeated runs are bitwise equal."""
    desc = model_examples.routenet(hidden=hidden, iterations=8)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("geant2", g) for g in range(2)])
    for gr in graphs:
        for f in mi.get_all_features():
            gr[f.name] = np.asarray(gr[f.name], np.float32) * np.float32(scale)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(11, bias_scale=0.2)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    errs = {}
    for seq, ro in (("2", "1"), ("6", "1"), ("2", "4"), ("6", "4"), ("2", "5"), ("6", "5")):
        monkeypatch.setenv("IGN_SEQ_VARIANT", seq)
        monkeypatch.setenv("IGN_READOUT_VARIANT", ro)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        b = Batch(eng, graphs)
        out = b.forward().reshape(-1)
        again = b.forward().reshape(-1)
        b.close()
        eng.close()
        assert np.array_equal(out, again)
        _close(out, ref)
        errs[seq + "/" + ro] = _scaled_err(out, ref)
    print("scale %g H %d: max scaled error vs float64 oracle (seq/readout variant):" % (scale, hidden), errs)
    for k, v in errs.items():
        assert v <= max(4 * errs["2/1"], 1e-6), errs


@pytest.mark.parametrize("order", ["routenet", "sum_first", "qsize"])
def test_fused_projection_matches_oracle(monkeypatch, order):
    """The 32-wide sum update projects its new states for the next ordered MP that reads them
    (sum_gru_g32's epilogue, IGN_FUSE_PROJ, default on): in RouteNet the link states of
    iteration t feed iteration t+1's path update; with the stages swapped the sum update runs
    first and the ordered update reads its result in the same iteration (the epilogue then also
    writes the table's hole row).  Fused and unfused forwards both match the float64 oracle, are
    deterministic, and differ (the switch took effect: the projection runs on split-bf16 instead
    of f32 MFMA)."""
    kind = "qsize" if order == "qsize" else "routenet"
    desc = model_examples.qsize(hidden=32, iterations=4) if kind == "qsize" else model_examples.routenet(hidden=32, iterations=4)
    if order == "sum_first":
        desc["message_passing"]["stages"] = desc["message_passing"]["stages"][::-1]
    _, dims, _ = workloads.model(kind)
    mi = Model_information(copy.deepcopy(desc), dims)
    # qsize: the {link, node} -> path interleave reads two sources, each projected by its own sum
    # update's epilogue (path -> link on the lane walk, path -> node on the segmented sum)
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("geant2", g, qsize=kind == "qsize")
                                            for g in range(3)])
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(13, bias_scale=0.2)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    outs = {}
    for v in ("0", "1"):
        monkeypatch.setenv("IGN_FUSE_PROJ", v)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        b = Batch(eng, graphs)
        out = b.forward().reshape(-1)
        np.testing.assert_array_equal(out, b.forward().reshape(-1))
        b.close()
        eng.close()
        _close(out, ref)
        outs[v] = out
    assert not np.array_equal(outs["0"], outs["1"])


@pytest.mark.parametrize("model", ["synthetic64", "routenet32"])
def test_split_bf16_sum_update_is_fp32_accurate(monkeypatch, model):
    """Sum-update variant 7 (x.W and h.U from exact 3-piece bf16 splits, 6 piece products:
    sum_gru_bf at DIN = H = 64, and at 32, sum_gru_g32 with its code-prefetched gather) and
    variant 8 (sum_gru_h16 at 64: scaled 2-piece fp16, 3 products; variant 7's kernel at 32)
    vs the f32-MFMA variant 3, on the synthetic graph's model and on RouteNet's path -> link
    update: both inside the parity tolerance vs the float64 oracle, the split form within 4x of
    the f32 error (or 1e-6); repeated runs are bitwise equal."""
    if model == "synthetic64":
        desc, dims, mi, graphs, _ = workloads.make_synthetic_inputs(n_nodes=3000, iterations=4, window=64)
    else:
        desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "geant2", 3)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(7, bias_scale=0.2)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    errs, outs = {}, {}
    for v in ("3", "7", "8"):
        monkeypatch.setenv("IGN_SUM_VARIANT", v)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        b = Batch(eng, graphs)
        out = b.forward().reshape(-1)
        np.testing.assert_array_equal(out, b.forward().reshape(-1))
        b.close()
        eng.close()
        _close(out, ref)
        errs[v], outs[v] = _scaled_err(out, ref), out
    print("max scaled error vs float64 oracle (sum variant):", errs)
    assert not np.array_equal(outs["3"], outs["7"])   # the variant switch took effect
    assert errs["7"] <= max(4 * errs["3"], 1e-6), errs
    assert errs["8"] <= max(4 * errs["3"], 1e-6), errs
    if model == "synthetic64":
        assert not np.array_equal(outs["7"], outs["8"])


@pytest.mark.parametrize("window", ["0", "1", "2", None])
def test_windowed_sum_matches_oracle(monkeypatch, window):
    """Windowed sum aggregation (per (graph, destination chunk) workgroups, source rows staged in
    LDS), the segmented sum (one wave per destination, IGN_SUM_WINDOW=2), forced off, and the
    default auto rule (for MPs with >= 64 messages per destination: Q-size's node update on
    synth50, ~140 per node) all match the float64 oracle.  The synth50 topology and batch shape of
    the Q-size bench, 6 graphs."""
    if window is None:
        monkeypatch.delenv("IGN_SUM_WINDOW", raising=False)
    else:
        monkeypatch.setenv("IGN_SUM_WINDOW", window)
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("qsize", "synth50", 6)
    if window == "0":   # every sum a lane walk: refused at >= 64 messages (Q-size's nodes carry 49-420)
        with pytest.raises(_lib.EngineError, match="IGN_SUM_WINDOW=0"):
            _run(desc, dims, graphs, seed=3, bias=0.1)
        return
    out, ref, b, _ = _run(desc, dims, graphs, seed=3, bias=0.1)
    _close(out, ref)
    np.testing.assert_array_equal(out, b.forward())


def _resident_vs_batched(monkeypatch, desc, dims, mi, graphs, mode="1", seed=5, bias=0.1, resident=True,
                         yardstick=False):
    """Runs the graphs with IGN_RESIDENT=mode and =0 (the batched launches): predictions and final
    states bitwise equal, both within TOL of the float64 oracle (yardstick: within _ieee_tol, IEEE
    float32's own error on these inputs), one resident launch per forward (plus the readout) where
    expected, replayed bitwise from the captured hipGraph.  Returns the resident run's
    ign_batch_resident_info."""
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(seed, bias_scale=bias)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    tol = _ieee_tol(plan, graphs, prm, ref) if yardstick else TOL
    outs, states, infos = {}, {}, {}
    for v in (mode, "0"):
        monkeypatch.setenv("IGN_RESIDENT", v)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        b = Batch(eng, graphs)
        eng.set_timing(True)
        out = b.forward().reshape(-1)
        st = eng.stats()
        eng.set_timing(False)
        np.testing.assert_array_equal(out, b.forward().reshape(-1))   # graph capture + replay
        if v != "0" and resident:
            assert st["mp_resident"]["launches"] == 1 and st["seq_gru"]["launches"] == 0, st
            assert st["sum_gru"]["launches"] == 0 and st["project"]["launches"] == 0, st
        else:
            assert st["mp_resident"]["launches"] == 0 and st["seq_gru"]["launches"] == plan.iterations, st
        infos[v] = b.resident_info()
        outs[v] = out
        states[v] = {e: b.state(e) for e in plan.entities}
        b.close()
        eng.close()
    assert infos[mode]["active"] == int(resident)
    np.testing.assert_array_equal(outs[mode], outs["0"])
    for e in plan.entities:
        np.testing.assert_array_equal(states[mode][e], states["0"][e])
    _close(outs[mode], ref, tol)
    return infos[mode]


@pytest.mark.parametrize("kind,topo,n,mode", [("routenet", "geant2", 3, "1"), ("routenet", "nsfnet", 2, "1"),
                                              ("routenet", "mixed", 4, "1"), ("routenet", "synth50", 2, "1"),
                                              ("routenet", "geant2", 2, "2"), ("qsize", "nsfnet", 2, "1"),
                                              ("qsize", "geant2", 2, "1"), ("qsize", "synth50", 2, "1"),
                                              ("qsize", "mixed", 3, "1"), ("qsize", "nsfnet", 2, "2")])
def test_resident_forward_is_the_batched_forward(monkeypatch, kind, topo, n, mode):
    """The graph-resident forward (resident.hip: one workgroup per graph for all T iterations;
    the default for RouteNet-shaped models and, since round 5, Q-size's interleave of links and
    nodes with its two sum MPs; synth50-size graphs, and every graph under IGN_RESIDENT=2, keep their
    path states in global memory, Q-size synth50 also its sum CSR) computes each row with the
    batched kernels' arithmetic: predictions and final states of every entity bitwise equal to the
    batched launches (IGN_RESIDENT=0), both within the parity tolerance of the float64 oracle."""
    if topo == "mixed":
        desc, dims, mi = workloads.model(kind)
        graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet" if g % 2 else "geant2", 40 + g,
                                                                          qsize=kind == "qsize") for g in range(n)])
    else:
        desc, dims, mi, graphs, _ = workloads.make_batch_inputs(kind, topo, n)
    # Q-size synth50: float32 itself (the IEEE build of oracle/cpu_forward.cpp) lies 8.3e-5 from the
    # float64 oracle on these two graphs (1.42e-4 over the x512 batch), so the case is
    # held to that yardstick, computed here on the same inputs
    info = _resident_vs_batched(monkeypatch, desc, dims, mi, graphs, mode,
                                yardstick=(kind, topo) == ("qsize", "synth50"))
    if topo == "synth50":   # RouteNet: path states in HBM / L2; Q-size: also the sum MPs' CSR
        assert info["form"] == (1 if kind == "routenet" else 2), info
    if mode == "2":
        assert info["form"] >= 1, info


@pytest.mark.parametrize("kind,topo,n,group", [("routenet", "geant2", 5, "2"), ("routenet", "nsfnet", 7, "3"),
                                               ("qsize", "geant2", 3, "2"), ("routenet", "mixed", 4, "4")])
def test_resident_graph_groups(monkeypatch, kind, topo, n, group):
    """IGN_RES_GROUP=K: one resident workgroup runs K consecutive graphs as one disjoint union (their
    path tiles claimed from one counter, their union-row tiles over all 16 waves), the last group
    short when K does not divide the batch: predictions and final states still bitwise the batched
    launches, one launch of ceil(n / K) workgroups."""
    monkeypatch.setenv("IGN_RES_GROUP", group)
    if topo == "mixed":
        desc, dims, mi = workloads.model(kind)
        graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet" if g % 2 else "geant2", 50 + g,
                                                                          qsize=kind == "qsize") for g in range(n)])
    else:
        desc, dims, mi, graphs, _ = workloads.make_batch_inputs(kind, topo, n)
    info = _resident_vs_batched(monkeypatch, desc, dims, mi, graphs)
    assert info["active"] == 1


def _routenet_graph(topo="nsfnet", gid=3, **kw):
    desc, dims, mi = workloads.model("routenet")
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample(topo, gid, **kw)])
    return desc, dims, mi, graphs[0]


def _with_holes(g, skip=0, count=3):
    """The ordered MP's positions of some multi-link paths (the count after the first skip) shifted
    up by one after their first link: a hole (a zero input below final_len, GM:477-490) at 1."""
    g = dict(g)
    dst = np.asarray(g["dst_adj_links_paths"])
    seq = np.asarray(g["seq_link_path"]).copy()
    multi = np.unique(dst[seq >= 1])
    assert multi.size >= skip + count
    for p in multi[skip:skip + count]:
        seq[(dst == p) & (seq >= 1)] += 1
    g["seq_link_path"] = list(seq)
    return g


def _with_idle_link(g):
    """One more link that no path crosses: its sum aggregates zero messages and the GRU still steps
    on x = 0 (AUX:752-765)."""
    g = dict(g)
    g["link_capacity"] = np.concatenate([np.asarray(g["link_capacity"], np.float32), np.float32([0.25])])
    g["num_link"] = int(g["num_link"]) + 1
    return g


@pytest.mark.parametrize("case", ["holes", "idle_link", "holes_idle_batch", "links_gt_256", "seg_every_row",
                                  "lane_walk_only", "lane_walk_refused", "qsize_holes"])
def test_resident_forward_edge_cases(monkeypatch, case):
    """The resident kernel's less common branches, each bitwise the batched launches and within the
    oracle's tolerance: a hole code (a sequence gap) at H = 32; a link with no message; a graph of
    260 links (17 union-row tiles: the GRU step and projection's second tile per wave); the
    segmented message sums for every row (IGN_SUM_WINDOW=2) and for none (0, which refuses a
    destination of >= 64 messages); Q-size's interleave with a hole and a dropped position."""
    if case == "qsize_holes":
        from tests.test_oracle import QS_DIMS, holes_input
        desc = model_examples.qsize(hidden=32, iterations=3)
        mi = Model_information(copy.deepcopy(desc), QS_DIMS)
        _resident_vs_batched(monkeypatch, desc, QS_DIMS, mi, [holes_input(), holes_input()], seed=7, bias=0.3)
        return
    if case == "links_gt_256":
        desc, dims, mi, g = _routenet_graph(n_nodes=20, n_links=130)
        assert g["num_link"] == 260
        info = _resident_vs_batched(monkeypatch, desc, dims, mi, [g])
        assert info["union_tiles"] == 17 and info["form"] == 1, info
        return
    if case == "seg_every_row":
        monkeypatch.setenv("IGN_SUM_WINDOW", "2")
        desc, dims, mi, g = _routenet_graph("geant2", 4)
        info = _resident_vs_batched(monkeypatch, desc, dims, mi, [g])
        assert info["seg_rows"] == g["num_link"], info
        return
    if case == "lane_walk_only":
        # every link's sum as a lane walk (GEANT2: at most 54 messages per link)
        monkeypatch.setenv("IGN_SUM_WINDOW", "0")
        desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "geant2", 2)
        info = _resident_vs_batched(monkeypatch, desc, dims, mi, graphs)
        assert info["seg_rows"] == 0, info
        return
    if case == "lane_walk_refused":
        # as lane walks, Q-size synth50's nodes (49-420 messages) landed at 4.3x IEEE
        # float32's error (round 5) and, below 128 messages, still at 1.8x (1.52e-4 against 8.3e-5,
        # gpurun_out r06_c07): the switch refuses a destination of >= 64 messages instead
        monkeypatch.setenv("IGN_SUM_WINDOW", "0")
        for kind in ("qsize", "routenet"):
            desc, dims, mi, graphs, _ = workloads.make_batch_inputs(kind, "synth50", 1)
            plan = MPPlan.from_model_info(mi)
            eng = Engine(plan, 0)
            eng.set_params(plan.init_params(5, bias_scale=0.1))
            with pytest.raises(_lib.EngineError, match="IGN_SUM_WINDOW=0"):
                Batch(eng, graphs)
            eng.close()
        return
    desc, dims, mi, g = _routenet_graph("nsfnet", 3)
    if case == "holes":
        graphs = [_with_holes(g)]
    elif case == "idle_link":
        graphs = [_with_idle_link(g)]
    else:
        _, _, _, g2 = _routenet_graph("geant2", 8)
        graphs = [_with_holes(g), g2, _with_idle_link(_with_holes(g2, skip=5, count=6))]
    _resident_vs_batched(monkeypatch, desc, dims, mi, graphs, seed=6, bias=0.2)


def test_resident_falls_back_beyond_16bit_rows(monkeypatch):
    """A graph of 66 000 paths over 8 links: its local path rows do not fit the resident tables'
    16 bits, so the batch runs the batched launches (ign_batch_resident_info: inactive), within the
    oracle's tolerance."""
    desc, dims, mi = workloads.model("routenet")
    rng = np.random.default_rng(11)
    P, L = 66000, 8
    lens = rng.integers(1, 4, P)
    dst_lp = np.repeat(np.arange(P), lens)
    seq_lp = np.concatenate([np.arange(k) for k in lens])
    links = np.concatenate([rng.permutation(L)[:k] for k in lens])
    order = np.lexsort((dst_lp, links))   # per link, its paths in path order
    g = {"link_capacity": rng.uniform(-1, 1, L).astype(np.float32), "traffic": rng.uniform(-1, 1, P).astype(np.float32),
         "src_adj_links_paths": list(links), "dst_adj_links_paths": list(dst_lp), "seq_link_path": list(seq_lp),
         "src_adj_paths_links": list(dst_lp[order]), "dst_adj_paths_links": list(links[order]),
         "seq_path_link": list(np.concatenate([np.arange(c) for c in np.bincount(links, minlength=L)])),
         "num_link": L, "num_path": P}
    _resident_vs_batched(monkeypatch, desc, dims, mi, [g], resident=False)


def test_segmented_sum_rule_is_per_destination(monkeypatch):
    """the segmented sum is chosen per destination (>= 64 messages), not from the batch's
    mean in-degree, so a Q-size synth50 graph (its nodes carry 49-420 messages) gets the same bits
    alone and in a batch with twelve NSFNET graphs (whose node MP averages < 64 per node), on the
    batched launches and on the resident forward."""
    desc, dims, mi = workloads.model("qsize")
    small = [synthetic.routenet_sample("nsfnet", 80 + g, qsize=True) for g in range(12)]
    big = synthetic.routenet_sample("synth50", 90, qsize=True)
    graphs, _ = workloads.graph_inputs(mi, small + [big])
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(8, bias_scale=0.1)
    n_big = graphs[-1]["num_path"]
    for v in ("0", "1"):
        monkeypatch.setenv("IGN_RESIDENT", v)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        alone = Batch(eng, graphs[-1:]).forward().reshape(-1)
        mixed = Batch(eng, graphs).forward().reshape(-1)
        np.testing.assert_array_equal(mixed[-n_big:], alone)
        eng.close()


@pytest.mark.parametrize("pg", ["0", "1"])
def test_resident_forward_batch_invariance(monkeypatch, pg):
    """A graph's predictions are the same bits alone, in a resident batch, and in a batch with a
    synth50 graph, too large for one workgroup's LDS: that batch runs the global-path form
    (IGN_RESIDENT_PG=1, default) or falls back to the batched launches (0)."""
    monkeypatch.setenv("IGN_RESIDENT_PG", pg)
    desc, dims, mi = workloads.model("routenet")
    small = [synthetic.routenet_sample("geant2", 60 + g) for g in range(3)]
    big = synthetic.routenet_sample("synth50", 70)
    graphs, _ = workloads.graph_inputs(mi, small + [big])
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(6, bias_scale=0.1))
    eng.set_timing(True)
    def launches():   # the stats accumulate over the engine's life
        st = eng.stats()
        return st["mp_resident"]["launches"], st["seq_gru"]["launches"]

    alone = [Batch(eng, [g]).forward().reshape(-1) for g in graphs[:3]]
    assert launches() == (3, 0)
    res = Batch(eng, graphs[:3]).forward().reshape(-1)
    assert launches() == (4, 0)
    mixed = Batch(eng, graphs).forward().reshape(-1)
    assert launches() == ((5, 0) if pg == "1" else (4, plan.iterations))
    np.testing.assert_array_equal(res, np.concatenate(alone))
    np.testing.assert_array_equal(mixed[:res.size], res)


@pytest.mark.parametrize("eager,defer", [("0", "1"), ("1", "0"), ("0", "0")])
def test_batch_build_switches_give_the_same_bits(monkeypatch, eager, defer):
    """The batch builder's round-5 defaults -- resident tables built in ign_batch_create
    (IGN_RESIDENT_EAGER=1) and host copies staged and waited for once per builder call
    (IGN_UPLOAD_DEFER=1) -- against building the tables at the first forward and waiting for every
    copy: predictions and the resident cost model identical, for RouteNet and Q-size batches."""
    for kind in ("routenet", "qsize"):
        desc, dims, mi, graphs, _ = workloads.make_batch_inputs(kind, "nsfnet", 3)
        plan = MPPlan.from_model_info(mi)
        prm = plan.init_params(4, bias_scale=0.1)
        outs, infos = [], []
        for e, d in (("1", "1"), (eager, defer)):
            monkeypatch.setenv("IGN_RESIDENT_EAGER", e)
            monkeypatch.setenv("IGN_UPLOAD_DEFER", d)
            eng = Engine(plan, 0)
            eng.set_params(prm)
            b = Batch(eng, graphs)
            outs.append(b.forward().reshape(-1))
            infos.append(b.resident_info())
            b.close()
            eng.close()
        np.testing.assert_array_equal(outs[0], outs[1])
        assert infos[0] == infos[1] and infos[0]["active"] == 1, infos


def test_timing_kinds_mask(monkeypatch):
    monkeypatch.setenv("IGN_RESIDENT", "0")   # the batched launches (the resident forward is one kind)
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "nsfnet", 2)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(0))
    b = Batch(eng, graphs)
    eng.set_timing(True, kinds=["seq_gru"])
    b.forward()
    st = eng.stats()
    assert st["seq_gru"]["launches"] == plan.iterations and st["seq_gru"]["ms"] > 0
    assert st["readout"]["launches"] == 0 and st["sum_gru"]["launches"] == 0


def test_training_records_no_timing(monkeypatch):
    """The training forward and the backward run the inference forward's MP step and readout head with
    a timer that never records: with every kind enabled they leave no launch in the statistics, and the
    inference forward after them still records its own."""
    import torch
    monkeypatch.setenv("IGN_RESIDENT", "0")   # the batched launches (the resident forward is one kind)
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs("routenet", "nsfnet", 2)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(0))
    b = Batch(eng, graphs)
    b.enable_training()
    eng.set_timing(True)
    b.forward_train()
    dpred = torch.ones(b.predictions * b.output_units, dtype=torch.float32, device="cuda")
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # torch's fills before the plan stream reads them
    b.backward(dpred, grads)
    torch.cuda.synchronize()
    st = eng.stats()
    assert {k: v["launches"] for k, v in st.items()} == {k: 0 for k in st}
    b.forward()
    assert eng.stats()["seq_gru"]["launches"] == plan.iterations
    b.close()
    eng.close()


# ---------------------------------------------------------------------------------------------
# schema-legal aggregations outside the example configs (AUX:264-401)
def _variant_inputs(desc, kind, n, seed0=0):
    _, dims, _ = workloads.model(kind)
    mi = Model_information(copy.deepcopy(desc), dims)
    samples = [synthetic.routenet_sample("nsfnet", seed0 + g, qsize=(kind == "qsize")) for g in range(n)]
    graphs, _ = workloads.graph_inputs(mi, samples)
    return dims, graphs


@pytest.mark.parametrize("aggr", [{"type": "attention"}, {"type": "convolution"},
                                  {"type": "convolution", "activation_function": "tanh"}])
@pytest.mark.parametrize("n", [1, 3])
def test_routenet_attention_convolution(aggr, n):
    desc = model_examples.routenet_aggregation(aggr, hidden=32, iterations=3)
    dims, graphs = _variant_inputs(desc, "routenet", n)
    out, ref, _, _ = _run(desc, dims, graphs, seed=5, bias=0.1)
    _close(out, ref)


@pytest.mark.parametrize("aggr", [{"type": "attention"}, {"type": "convolution"}])
def test_two_source_attention_convolution(aggr):
    """{link, node} -> path: the combined edge list and the attention position quirk (GM:539-541)."""
    desc = model_examples.qsize_aggregation(aggr, iterations=3)
    dims, graphs = _variant_inputs(desc, "qsize", 2)
    out, ref, _, _ = _run(desc, dims, graphs, seed=6, bias=0.1)
    _close(out, ref)


@pytest.mark.parametrize("axis", [1, 2])
def test_two_source_concat(axis):
    """{link, node} -> path concatenated on axis 1 (slots) or 2 (features, AUX:443-456): the
    axis-2 step input is [link message | node message], final_len the first source's lens."""
    desc = model_examples.qsize_aggregation({"type": "concat", "concat_axis": axis}, iterations=3)
    dims, graphs = _variant_inputs(desc, "qsize", 2)
    out, ref, _, _ = _run(desc, dims, graphs, seed=7, bias=0.1)
    _close(out, ref)


# ---------------------------------------------------------------------------------------------
# message-creation networks (GM:440-475)
def _with_edge_params(sample, rng):
    s = copy.deepcopy(sample)
    s["adj_paths_links"] = {l: [[p, [float(rng.uniform(0, 1)), float(rng.uniform(-1, 1))]] for p in ps]
                            for l, ps in s["adj_paths_links"].items()}
    return s


@pytest.mark.parametrize("inputs,units", [(("hs_source", "hs_dest"), (48, 32)), (("hs_source",), (32,)),
                                          (("hs_dest", "hs_source", "edge_params"), (32,))])
def test_message_network_sum_mp(inputs, units):
    from ignnition_amd.framework_operations import dimensions_of_sample
    rng = np.random.default_rng(0)
    desc = model_examples.routenet_message_net(inputs=inputs, units=units, activation="selu", iterations=3)
    samples = [synthetic.routenet_sample("nsfnet", g) for g in range(2)]
    if "edge_params" in inputs:
        samples = [_with_edge_params(s, rng) for s in samples]
    dims = dimensions_of_sample(samples[0])
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, _ = workloads.graph_inputs(mi, samples)
    out, ref, _, _ = _run(desc, dims, graphs, seed=8, bias=0.1)
    _close(out, ref)


def test_message_network_ordered_mp():
    """A network on the link -> path (ordered) messages: the projected table is per edge."""
    desc = model_examples.routenet(iterations=3)
    src = desc["message_passing"]["stages"][0]["stage_mp"][0]["source_entities"][0]
    src["message"] = [{"type": "neural_network", "nn_name": "message_nn", "input": ["hs_source", "hs_dest"]}]
    desc["neural_networks"].append({"nn_name": "message_nn", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dense", "units": 32, "activation": "tanh"}]})
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", g) for g in range(2)])
    out, ref, _, _ = _run(desc, dims, graphs, seed=9, bias=0.1)
    _close(out, ref)


# ---------------------------------------------------------------------------------------------
# readout operations before predict (GM:605-655, AUX:1033-1265)
from tests.readout_cases import READOUT_CASES, _POOL  # noqa: E402


@pytest.mark.parametrize("case", sorted(READOUT_CASES))
@pytest.mark.parametrize("n", [1, 3])
def test_readout_operations(case, n):
    ops, pin, nets = READOUT_CASES[case]
    desc = model_examples.routenet_readout(ops, pin, nets, iterations=3)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet" if g % 2 == 0 else "geant2", g)
                                            for g in range(n)])
    out, ref, b, _ = _run(desc, dims, graphs, seed=11, bias=0.1)
    _close(out, ref)
    assert int(b.graph_predictions.sum()) * b.output_units == out.size


@pytest.mark.parametrize("kind", ["sum", "mean", "max"])
def test_pooling_many_chunks(kind):
    """Graph-level prediction on a 20 000-node graph: the pooling kernel reduces 5 chunks of
    rows per graph, then the chunk partials in a fixed order."""
    desc, dims, mi, graphs, _ = workloads.make_synthetic_inputs(n_nodes=20000, iterations=2, window=64)
    pred = desc["readout"][0]
    pred["input"] = ["g"]
    desc["readout"] = [_POOL(kind, "node", "g"), pred]
    out, ref, b, _ = _run(desc, dims, graphs, seed=5, bias=0.1)
    _close(out, ref)
    assert out.size == 1


@pytest.mark.parametrize("kind", ["routenet", "qsize"])
def test_json_plan_forward_matches_python_plan(kind):
    """A plan from ign_plan_create_json (the C++ lowering of model_description.json) runs the
    same forward as the Python-lowered plan: bitwise-equal predictions."""
    import ctypes as C
    import json
    desc, dims, mi, graphs, _ = workloads.make_batch_inputs(kind, "nsfnet", 2)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(3, bias_scale=0.1)
    e1 = Engine(plan, 0)
    e1.set_params(prm)
    ref = Batch(e1, graphs).forward()
    e2 = Engine(plan, 0)
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h)))
    _lib.lib.ign_plan_destroy(e2.handle)
    e2.handle = h
    e2.set_params(prm)
    np.testing.assert_array_equal(Batch(e2, graphs).forward(), ref)


# ---------------------------------------------------------------------------------------------
# ABI 13: int32 index arrays (ign_batch_desc.index_bytes = 4)
def _narrowed(graphs):
    from ignnition_amd.engine import BatchedGraphs
    bg = BatchedGraphs.from_dicts(graphs)
    return BatchedGraphs({k: (v.astype(np.int32) if v.dtype == np.int64 else v, lens)
                          for k, (v, lens) in bg.arrays.items()}, bg.num_graphs)


@pytest.mark.parametrize("case", ["routenet", "qsize", "extend_nn"])
def test_int32_index_batches_equal_int64(case):
    """A batch whose index arrays are int32 (index_bytes 4: the native reader's narrow gather hands
    them over without widening) predicts bitwise what the int64 batch predicts: RouteNet, Q-size
    (interleave indices) and a readout with extend_adjacencies (readout.cpp reads the desc too)."""
    if case == "extend_nn":
        ops, pin, nets = READOUT_CASES[case]
        desc = model_examples.routenet_readout(ops, pin, nets, iterations=3)
        _, dims, _ = workloads.model("routenet")
        mi = Model_information(copy.deepcopy(desc), dims)
        graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet" if g % 2 == 0 else "geant2", g)
                                                for g in range(3)])
    else:
        desc, dims, mi, graphs, _ = workloads.make_batch_inputs(case, "geant2", 3)
    plan = MPPlan.from_model_info(mi)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(5, bias_scale=0.1))
    outs = []
    for g in (graphs, _narrowed(graphs)):
        b = Batch(eng, g)
        outs.append(b.forward().reshape(-1).copy())
        b.close()
    eng.close()
    assert outs[0].size > 0
    np.testing.assert_array_equal(outs[0], outs[1])


def test_native_narrow_gather_batches_equal_wide(tmp_path):
    """The training input path (NativeInput.load: the native reader's narrow gather) builds batches
    that predict bitwise what the wide (int64) gather's batches predict."""
    from ignnition_amd.dataset import NativeDataset, plan_keys
    desc, dims, mi = workloads.model("qsize")
    synthetic.write_tar_dataset(synthetic.dataset("nsfnet", 5, qsize=True), str(tmp_path), per_file=3)
    ds = NativeDataset.for_model(str(tmp_path), mi)
    plan = MPPlan.from_model_info(mi)
    keys = plan_keys(plan)
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(2, bias_scale=0.1))
    outs = []
    for narrow in (False, True):
        bg, _ = ds.batch([3, 1, 4, 0], keys, narrow=narrow)
        assert any(bg.get(k)[0].dtype == np.int32 for k in keys) == narrow
        b = Batch(eng, bg)
        outs.append(b.forward().reshape(-1).copy())
        b.close()
    eng.close()
    ds.close()
    np.testing.assert_array_equal(outs[0], outs[1])
