"""LayerNormalization cases shared by the host and the GPU tests: descriptions built from
tests/predict_cases with LayerNormalization (and Dropout) layers inserted, and the float64 autograd
oracle whose readout Dense stacks apply them.  The oracle's LayerNormalization is Keras' on a 2-D
[rows, units] input, written from its definition: mean = sum(x) / units, var = sum((x - mean)^2) /
units, y = (x - mean) * (1 / sqrt(var + epsilon)) * gamma + beta."""
import copy

import numpy as np

from tests import dropout_cases as dc
from tests.predict_cases import layer_name, predict_model

LN = "LayerNormalization"


def ln(**options):
    return dict({"type_layer": LN}, **options)


def drop(rate, **options):
    return dict({"type_layer": "Dropout", "rate": rate}, **options)


def insert_layers(desc, layers, nn_name="readout_model"):
    """``desc`` with further layers in network ``nn_name``: layers = [(before_dense, layer)], in the
    order they are to stand; before_dense = the index of the Dense layer a layer precedes (the Dense
    count: after the last)."""
    desc = copy.deepcopy(desc)
    for net in desc["neural_networks"]:
        if net["nn_name"] != nn_name:
            continue
        dense = net["nn_architecture"]
        arch = []
        for l in range(len(dense) + 1):
            arch += [copy.deepcopy(layer) for b, layer in layers if b == l]
            if l < len(dense):
                arch.append(dense[l])
        net["nn_architecture"] = arch
    return desc


def ln_model(case, layers, **kw):
    return insert_layers(predict_model(case, **kw), layers)


def width_model(units):
    """Dense(units, tanh), LayerNormalization, Dense(1): the layer at width ``units``."""
    desc = predict_model("one_layer")
    for net in desc["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"] = [
                {"type_layer": "Dense", "name": layer_name(0), "units": units, "activation": "tanh"},
                ln(name="ln"),
                {"type_layer": "Dense", "name": layer_name(1), "units": 1, "activation": "None"}]
    return desc


def last_model(units, activation="tanh"):
    """Dense(8, tanh), Dense(units, activation), LayerNormalization: the predictions are the layer's output."""
    desc = predict_model("one_layer")
    for net in desc["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"] = [
                {"type_layer": "Dense", "name": layer_name(0), "units": 8, "activation": "tanh"},
                {"type_layer": "Dense", "name": layer_name(1), "units": units, "activation": activation},
                ln(name="ln")]
    return desc


_POOL = {"type": "pooling", "type_pooling": "sum", "input": ["pe"], "output_name": "g"}
_EMB = {"type": "neural_network", "nn_name": "emb", "input": ["path"], "output_name": "pe"}


def pooled_model():
    """Predict on the pooled graph rows (one row per graph: fewer rows than one wave's row group), a
    LayerNormalization of width 16 first in predict and one of width 24 inside the operation."""
    desc = predict_model("two_layer", ops=[_EMB, _POOL], predict_input=("g",))
    desc["neural_networks"].append({"nn_name": "emb", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dense", "units": 24, "activation": "tanh"},
        ln(),
        {"type_layer": "Dense", "units": 16, "activation": "selu"}]})
    return insert_layers(desc, [(0, ln(name="ln_first"))])


def nn_two_inputs_first_model():
    """A LayerNormalization in front of layer 0 of a readout neural_network operation with two inputs:
    the stack's input gradient goes through the concat scratch."""
    desc = predict_model("two_layer", ops=[dict(_EMB, input=["path", "path"]), _POOL], predict_input=("g",))
    desc["neural_networks"].append({"nn_name": "emb", "nn_type": "feed_forward", "nn_architecture": [
        ln(),
        {"type_layer": "Dense", "units": 24, "activation": "tanh"},
        {"type_layer": "Dense", "units": 16, "activation": "selu"}]})
    return desc


def degenerate_model(last):
    """A relu Dense layer of 16 units in front of the LayerNormalization; with its bias at -1e3 every
    row it writes is zero.  last: the layer's output is the prediction; else a Dense(1) follows."""
    desc = predict_model("one_layer")
    for net in desc["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"] = [
                {"type_layer": "Dense", "name": layer_name(0), "units": 16, "activation": "relu"},
                ln(name="ln")] + ([] if last else [
                    {"type_layer": "Dense", "name": layer_name(1), "units": 1, "activation": "None"}])
    return desc


def tail_chain_model():
    """Dense(8, tanh), Dense(24, tanh), then LayerNormalization, Dropout(0.25), LayerNormalization after
    the last Dense layer: three chained layers behind the stack's output."""
    desc = last_model(24)
    for net in desc["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"] += [drop(0.25), ln(name="ln2")]
    return desc


def first_acc_path_model():
    """A single-input readout operation on the path states with the layer first, and predict reading the
    operation's output beside the path states: the layer's input gradient is added to the path gradient
    that predict's backward already wrote (width 32)."""
    desc = predict_model("odd_widths", ops=[_EMB], predict_input=("pe", "path"))
    desc["neural_networks"].append({"nn_name": "emb", "nn_type": "feed_forward", "nn_architecture": [
        ln(),
        {"type_layer": "Dense", "units": 24, "activation": "tanh"},
        {"type_layer": "Dense", "units": 16, "activation": "selu"}]})
    return desc


def first_acc_model(width):
    """The same at another width: pe = Dense(width, tanh)(path); a second single-input operation with the
    layer first reads pe; predict reads its output beside pe, so the layer's input gradient is added to
    rows of `width` floats that already hold predict's gradient."""
    emb2 = {"type": "neural_network", "nn_name": "emb2", "input": ["pe"], "output_name": "pe2"}
    desc = predict_model("odd_widths", ops=[_EMB, emb2], predict_input=("pe2", "pe"))
    desc["neural_networks"].append({"nn_name": "emb", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dense", "units": width, "activation": "tanh"}]})
    desc["neural_networks"].append({"nn_name": "emb2", "nn_type": "feed_forward", "nn_architecture": [
        ln(),
        {"type_layer": "Dense", "units": 16, "activation": "selu"}]})
    return desc


GRAD_CASES = {
    # the layer after the last Dense layer at a width above 1 (16 lanes per row, float4, wide), and chained there
    "last_7": lambda: last_model(7),
    "last_256": lambda: last_model(256),
    "last_300": lambda: last_model(300),
    "tail_chain_24": tail_chain_model,
    # the layer first in a single-input stack: its input gradient is added to the input tensor's
    # (32 lanes per row; the strided, float4 and wide forms on rows that already hold a gradient)
    "first_path": lambda: ln_model("two_layer", [(0, ln())]),
    "first_acc_path": first_acc_path_model,
    "first_acc_100": lambda: first_acc_model(100),
    "first_acc_256": lambda: first_acc_model(256),
    "first_acc_300": lambda: first_acc_model(300),
    "four_layer": lambda: ln_model("four_layer", [(1, ln()), (3, ln(name="ln_b"))]),
    "odd_widths_first_last": lambda: ln_model("odd_widths", [(0, ln()), (3, ln())]),
    "nn_two_inputs_first": nn_two_inputs_first_model,
    "with_dropout": lambda: ln_model("four_layer", [(1, ln()), (1, drop(0.5)), (3, drop(0.25, seed=4)), (3, ln())]),
    "no_affine_eps_1e-5": lambda: ln_model("four_layer", [(1, ln(center=False, scale=False, epsilon=1e-5))]),
}


def inputs(desc, n_graphs=2, seed=dc.SEED):
    """dropout_cases.inputs; predictions of several units per path take labels [paths][units] from a
    fixed RNG (the loss is the mean over the flat predictions)."""
    dims, plan, graphs, labels, prm = dc.inputs(desc, n_graphs=n_graphs, seed=seed)
    units = plan.dense[-1][1]
    if units > 1 and plan.predict_space[0] == "entity":
        rng = np.random.default_rng(5)
        labels = [rng.normal(size=(int(np.asarray(g["num_path"])), units)).astype(np.float32) for g in graphs]
    return dims, plan, graphs, labels, prm


def make_oracle(desc, dims, prm, plan, graphs, seed=0, step=0):
    """TorchOracle whose readout Dense stacks run LayerNormalization layers, and Dropout layers with
    the ign_dropout_keep masks of (seed, step); only ``_readout`` is overridden.  ``min_var`` holds,
    per (readout-list counter, layer index), the smallest row variance that entered the layer."""
    import torch
    from oracle.train_oracle import TorchOracle, _act

    rows = {}   # rows per graph of each stack's input space
    for stack in {s[1] for s in plan.dropout_sites()}:
        space = plan.predict_space if stack < 0 else plan.ro_spaces[plan.readout_ops[stack]["inputs"][0]]
        assert space[0] in ("entity", "graph")
        rows[stack] = [int(np.asarray(g["num_" + plan.entities[space[1]]])) if space[0] == "entity" else 1 for g in graphs]
    masks = {k: torch.tensor(v, dtype=torch.float64)
             for k, v in dc.site_masks(plan, lambda s: sum(rows[s]), seed, step).items()}
    op_stack = {op["counter"]: k for k, op in enumerate(plan.readout_ops)}
    op_stack[plan.predict_counter] = -1

    class LayerNormOracle(TorchOracle):
        _graph = 0   # forward() walks the graphs in order, one _readout each
        min_var = {}

        def _layer_norm(self, h, layer, pre, key):
            units = h.shape[1]
            mean = h.sum(1, keepdim=True) / units
            var = ((h - mean) ** 2).sum(1, keepdim=True) / units
            self.min_var[key] = min(self.min_var.get(key, np.inf), float(var.min().detach()))
            y = (h - mean) * (1.0 / torch.sqrt(var + float(layer.get("epsilon", 1e-3))))
            if layer.get("scale", True):
                y = y * self.p[pre + "/gamma"]
            if layer.get("center", True):
                y = y + self.p[pre + "/beta"]
            return y

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
                dense, seen = 0, {}
                for li, layer in enumerate(self.nn[op["nn_name"]]["nn_architecture"]):
                    name = layer.get("name", "layer_%d_%s_readout" % (li, layer["type_layer"]))
                    pre = "readout_model_%d/%s" % (counter, name)
                    if layer["type_layer"] == "Dropout":
                        if float(layer["rate"]) > 0:
                            k = seen.get(dense, 0)
                            seen[dense] = k + 1
                            r0 = sum(rows[stack][:self._graph])
                            h = h * masks[stack, dense, k][r0:r0 + h.shape[0]]
                        continue
                    if layer["type_layer"] == LN:
                        h = self._layer_norm(h, layer, pre, (counter, li))
                        continue
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

    ora = LayerNormOracle(desc, dims, prm)
    ora.min_var = {}
    return ora
