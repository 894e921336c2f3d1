"""Dropout cases shared by the host and the GPU tests: descriptions built from tests/predict_cases
with Dropout layers inserted, a numpy restatement of the mask (Philox4x32-10, written from the
published algorithm), and the float64 autograd oracle with the masks applied."""
import copy

import numpy as np

from ignnition_amd import workloads
from ignnition_amd.engine import MPPlan, dropout_keep
from ignnition_amd.json_operations import Model_information
from tests.predict_cases import BIAS, SEED, predict_model

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 uint64 arrays holding 32-bit words, key: 2 such; returns the 4 output word arrays."""
    c = [np.asarray(x, np.uint64) & M32 for x in ctr]
    k = [np.asarray(x, np.uint64) & M32 for x in key]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return c


def keep_numpy(seed, site, step, rows, units, rate):
    """The keep mask [rows, units] restated: counter (g low, g high, site, step), g = i >> 2, key
    (seed low, seed high), word i & 3, u = (word >> 8) * 2^-24, keep = u >= rate in float32."""
    i = np.arange(rows * units, dtype=np.uint64)
    g = i >> np.uint64(2)
    z = np.zeros_like(g)
    w = philox4x32_10([g & M32, g >> np.uint64(32), z + np.uint64(site), z + np.uint64(step)],
                      [z + np.uint64(seed & 0xFFFFFFFF), z + np.uint64(seed >> 32)])
    word = np.choose((i & np.uint64(3)).astype(np.int64), w)
    u = (word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(rate)).reshape(rows, units).astype(np.uint8)


def insert_dropout(desc, sites, nn_name="readout_model"):
    """``desc`` with Dropout layers in network ``nn_name``: sites = [(before_dense, rate, options)],
    before_dense = the index of the Dense layer it precedes (the Dense count: after the last)."""
    desc = copy.deepcopy(desc)
    for net in desc["neural_networks"]:
        if net["nn_name"] != nn_name:
            continue
        dense = net["nn_architecture"]
        arch = []
        for l in range(len(dense) + 1):
            arch += [dict({"type_layer": "Dropout", "rate": r}, **opt) for b, r, opt in sites if b == l]
            if l < len(dense):
                arch.append(dense[l])
        net["nn_architecture"] = arch
    return desc


def dropout_model(case, sites, **kw):
    return insert_dropout(predict_model(case, **kw), sites)


_POOL = {"type": "pooling", "type_pooling": "sum", "input": ["pe"], "output_name": "g"}
_EMB = {"type": "neural_network", "nn_name": "emb", "input": ["path"], "output_name": "pe"}


def readout_op_model(rate=0.5):
    """A readout neural_network operation holding a Dropout between its two Dense layers and one after
    the last, then pooling, then predict (two_layer) on the pooled row."""
    desc = predict_model("two_layer", ops=[_EMB, _POOL], predict_input=("g",))
    desc["neural_networks"].append({"nn_name": "emb", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dense", "units": 24, "activation": "tanh"},
        {"type_layer": "Dropout", "rate": rate},
        {"type_layer": "Dense", "units": 16, "activation": "selu"},
        {"type_layer": "Dropout", "rate": 0.25, "seed": 5}]})
    return desc


def nn_two_inputs_first_model():
    """A Dropout in front of layer 0 of a readout neural_network operation with two inputs: the stack's
    input gradient is written to the concat scratch, masked in place, then split by columns."""
    desc = predict_model("two_layer", ops=[dict(_EMB, input=["path", "path"]), _POOL], predict_input=("g",))
    desc["neural_networks"].append({"nn_name": "emb", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dropout", "rate": 0.25},
        {"type_layer": "Dense", "units": 24, "activation": "tanh"},
        {"type_layer": "Dense", "units": 16, "activation": "selu"}]})
    return desc


def predict_two_inputs_first_model():
    """The same in predict (odd_widths), reading the operation's output beside the path states."""
    desc = predict_model("odd_widths", ops=[_EMB], predict_input=("pe", "path"))
    desc["neural_networks"].append({"nn_name": "emb", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dense", "units": 16, "activation": "tanh"}]})
    return insert_dropout(desc, [(0, 0.25, {})])


def inputs(desc, n_graphs=2, seed=SEED):
    """(dims, plan, graphs, labels, parameters) for NSFNET samples 0 .. n_graphs - 1, as
    predict_cases.predict_inputs; labels shaped like the predictions when they are per graph."""
    from ignnition_amd import synthetic
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", g) for g in range(n_graphs)])
    plan = MPPlan.from_model_info(mi)
    if plan.predict_space[0] == "graph":
        rng = np.random.default_rng(5)
        labels = [rng.normal(size=plan.dense[-1][1]).astype(np.float32) for _ in graphs]
    return dims, plan, graphs, labels, plan.init_params(seed, bias_scale=BIAS)


def site_masks(plan, rows_of_stack, seed, step):
    """{(stack, ordinal in the stack): float64 keep * scale [rows, units]} from ign_dropout_keep, for the
    plan's sites; rows_of_stack(stack) = the batch's rows of the stack's input space."""
    out, count = {}, {}
    for site, stack, before, rate, lseed in plan.dropout_sites():
        layers = plan.dense if stack < 0 else plan.readout_ops[stack]["layers"]
        if before < len(layers):
            units = (layers[before - 1][1] if before else
                     sum(plan.ro_widths[i] for i in (plan.readout_inputs if stack < 0 else plan.readout_ops[stack]["inputs"])))
        else:
            units = layers[-1][1]
        keep = dropout_keep(seed ^ lseed, site, step, rows_of_stack(stack), units, rate)
        scale = np.float64(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))
        k = count.get((stack, before), 0)
        count[stack, before] = k + 1
        out[stack, before, k] = keep.astype(np.float64) * scale
    return out


def make_oracle(desc, dims, prm, plan, graphs, seed, step):
    """TorchOracle whose readout Dense stacks multiply by the ign_dropout_keep masks and the float32
    scale (tf.nn.dropout with training=True); only ``_readout`` is overridden."""
    import torch
    from oracle.train_oracle import TorchOracle, _act

    rows = {}   # rows per graph of each stack's input space
    for stack in {s[1] for s in plan.dropout_sites()}:
        space = plan.predict_space if stack < 0 else plan.ro_spaces[plan.readout_ops[stack]["inputs"][0]]
        if space[0] == "entity":
            rows[stack] = [int(np.asarray(g["num_" + plan.entities[space[1]]])) for g in graphs]
        elif space[0] == "graph":
            rows[stack] = [1] * len(graphs)
        else:
            rows[stack] = [len(np.asarray(g[plan.adj_slots[space[1]].keys[0]]).reshape(-1)) for g in graphs]
    masks = {k: torch.tensor(v, dtype=torch.float64)
             for k, v in site_masks(plan, lambda s: sum(rows[s]), seed, step).items()}
    op_stack = {}   # readout-list counter -> the plan's readout-op index
    for k, op in enumerate(plan.readout_ops):
        op_stack[op["counter"]] = k
    op_stack[plan.predict_counter] = -1

    class DropoutOracle(TorchOracle):
        _graph = 0   # forward() walks the graphs in order, one _readout each

        def _mask(self, h, stack, before, k):
            r0 = sum(rows[stack][:self._graph])
            return h * masks[stack, before, k][r0:r0 + h.shape[0]]

        def _readout(self, state, x):
            var = dict(state)
            for counter, op in enumerate(self.d["readout"]):
                t = op["type"]
                if t == "pooling" and op["type_pooling"] in ("sum", "mean"):   # AUX:1165-1185
                    v = var[op["input"][0]]
                    r = v.sum(0) if op["type_pooling"] == "sum" else v.sum(0) / v.shape[0]
                    var[op["output_name"]] = r.reshape(1, -1)
                    continue
                assert t in ("predict", "neural_network"), "readout operation %r is not restated here" % t
                stack = op_stack[counter]
                h = torch.cat([var[i] for i in op["input"]], 1)
                dense = 0
                seen = {}
                for li, layer in enumerate(self.nn[op["nn_name"]]["nn_architecture"]):
                    if layer["type_layer"] == "Dropout":
                        if float(layer["rate"]) > 0:
                            k = seen.get(dense, 0)
                            seen[dense] = k + 1
                            h = self._mask(h, stack, dense, k)
                        continue
                    name = layer.get("name", "layer_%d_%s_readout" % (li, layer["type_layer"]))
                    pre = "readout_model_%d/%s" % (counter, name)
                    h = h @ self.p[pre + "/kernel"]
                    if pre + "/bias" in self.p:
                        h = h + self.p[pre + "/bias"]
                    h = _act(h, layer.get("activation"))
                    dense += 1
                if t == "predict":
                    self._graph = (self._graph + 1) % len(graphs)
                    return h
                var[op.get("output_name", "None")] = h
            raise AssertionError("no predict operation")

    return DropoutOracle(desc, dims, prm)
