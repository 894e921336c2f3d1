"""Lowering of a ``Model_information`` plan to the C ABI, parameters and batches.

``MPPlan`` is the counterpart of ``ComnetModel.__init__`` (GM:235-382): it walks the MP
stages in order and decides, per message passing, the aggregation, the GRU cell of the
destination (one per destination entity name, GM:309-313) and the adjacency arrays each
source reads (``src_/dst_<adj>``, ``seq_<src>_<dst>``, ``indices_<src>_to_<dst>``, exactly
the keys of input_fn, GM:127-158).  ``Batch`` turns a list of per-graph feature dicts
into one disjoint-union batch on the device.

Parameters use Keras-style names so checkpoints read like the reference's variables:
``<dst>_update/kernel`` [in, 3H], ``<dst>_update/recurrent_kernel`` [H, 3H],
``<dst>_update/bias`` [2, 3H], ``readout_model_0/<layer>/kernel`` / ``bias``.
"""

from __future__ import annotations

import atexit
import ctypes as C
import weakref
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import check, lib

SUPPORTED_GRU_KEYS = {"units", "name"}
# the GRUCell keys lowered beside them (ign_plan_set_cell_options), with the Keras GRUCell v2 defaults
GRU_OPTION_DEFAULTS = {"activation": "tanh", "recurrent_activation": "sigmoid", "use_bias": True, "reset_after": True}


def _gru_options(parameters):
    """(activation code, recurrent_activation code, use_bias, reset_after) of a GRU cell's parameters."""
    extra = set(parameters) - SUPPORTED_GRU_KEYS - set(GRU_OPTION_DEFAULTS)
    if extra:
        raise UnsupportedModel("GRU options %s are not lowered (Keras defaults only)" % sorted(extra))
    prm = dict(GRU_OPTION_DEFAULTS, **{k: v for k, v in parameters.items() if k in GRU_OPTION_DEFAULTS})
    codes = []
    for key in ("activation", "recurrent_activation"):
        if prm[key] is not None and not isinstance(prm[key], str):   # (a list or dict: plan_json.cpp's text)
            raise ValueError("GRU %s: expected a string" % key)
        if prm[key] not in _lib.ACT:
            raise UnsupportedModel("activation %r not supported" % prm[key])
        codes.append(_lib.ACT[prm[key]])
    return codes[0], codes[1], bool(prm["use_bias"]), bool(prm["reset_after"])

# Live handles, released explicitly at interpreter exit (batches before plans) while the HIP
# runtime is still up; relying on __del__ during module teardown can run after it is gone.
_LIVE_BATCHES: "weakref.WeakSet" = weakref.WeakSet()
_LIVE_ENGINES: "weakref.WeakSet" = weakref.WeakSet()


@atexit.register
def _release_all():
    for b in list(_LIVE_BATCHES):
        b.close()
    for e in list(_LIVE_ENGINES):
        e.close()


class UnsupportedModel(ValueError):
    pass


@dataclass
class AdjSlot:
    adj: str
    src: str
    dst: str

    @property
    def keys(self):
        return "src_" + self.adj, "dst_" + self.adj, "seq_" + self.src + "_" + self.dst


def _message_net(s, dst, plan, eidx):
    """The message-creation network of one MP source (GM:440-475), or None (direct_assignation).
    The reference builds every network of a source under one name (its counter counts sources,
    GM:251/281) and reads chained outputs under another (GM:458 vs 470), so exactly one network
    per source reading hs_source / hs_dest / edge_params is what it can run."""
    nets = [op for op in s.message_formation if op.type != "direct_assignation"]
    if not nets:
        return None
    if len(nets) > 1:
        raise UnsupportedModel("more than one message network per source (the reference cannot chain them, GM:458/470)")
    op = nets[0]
    inputs = list(getattr(op, "input", []))
    for name in inputs:
        if name not in _lib.MSG_INPUT:
            raise UnsupportedModel("message input %r is not readable in the reference (GM:458/470)" % name)
    layers = []
    for l in op.model.layers:
        if l.type == "Dropout":
            raise UnsupportedModel("message layer type Dropout is not lowered: a message-creation network would need a "
                                   "fresh mask per iteration (Dropout is lowered in the readout's Dense stacks only)")
        if l.type != "Dense":
            raise UnsupportedModel("message layer type %s is not lowered (Dense only)" % l.type)
        prm = dict(l.parameters)
        act = prm.get("activation", None)
        if act not in _lib.ACT or act in _lib.ACT_REFUSED_AT["message"]:
            raise UnsupportedModel("activation %r not supported" % act)
        known = {"units", "activation", "kernel_regularizer", "name", "use_bias"}
        if set(prm) - known:
            raise UnsupportedModel("Dense options %s are not lowered" % sorted(set(prm) - known))
        layers.append((prm.get("name"), int(prm["units"]), _lib.ACT[act], int(bool(prm.get("use_bias", True))),
                       float(prm.get("kernel_regularizer", 0.0) or 0.0)))
    widths = {"hs_source": plan.hidden[eidx[s.name]], "hs_dest": plan.hidden[eidx[dst]],
              "edge_params": int(s.extra_parameters)}
    return {"prefix": "%s_to_%s_message_creation_0/" % (s.name, dst), "inputs": inputs,
            "param_dim": int(s.extra_parameters), "din": sum(widths[i] for i in inputs), "layers": layers}


@dataclass
class MPPlan:
    """The lowered plan (entities, adjacency slots, MPs, cells, readout)."""
    model_info: object
    entities: list = field(default_factory=list)       # names
    hidden: list = field(default_factory=list)
    features: list = field(default_factory=list)       # [(name, size)] per entity
    adj_slots: list = field(default_factory=list)
    il_slots: list = field(default_factory=list)       # indices_<src>_to_<dst> keys
    mps: list = field(default_factory=list)            # dicts
    cells: list = field(default_factory=list)          # [(dst_name, din, H)]
    cell_options: list = field(default_factory=list)   # per cell: (activation, recurrent_activation, use_bias, reset_after)
    readout_inputs: list = field(default_factory=list)  # predict inputs: readout tensor ids
    readout_ops: list = field(default_factory=list)     # operations before predict (dicts)
    ro_widths: list = field(default_factory=list)       # readout tensor widths (entity states first)
    ro_spaces: list = field(default_factory=list)       # row space per tensor: ("entity", e) / ("graph",) / ("adj", slot)
    predict_counter: int = 0                           # readout_model_<index of predict in the readout list>
    dense: list = field(default_factory=list)          # [(name, units, act, use_bias, l2)]
    extra: list = field(default_factory=list)          # predict's Dropout and LayerNormalization layers in the
                                                       # architecture's order (_dense_layers)
    iterations: int = 0
    readout_label: str = ""
    convolution_dim: int = 0                           # F of convolution/kernel [F, F] (0: none)
    attention_dim: int = 0                             # F of the attention weights (0: none)

    @classmethod
    def from_model_info(cls, mi) -> "MPPlan":
        p = cls(model_info=mi)
        p.iterations = mi.get_mp_iterations()
        for e in mi.get_entities():
            p.entities.append(e.name)
            h = int(e.hidden_state_dimension)
            if h != e.hidden_state_dimension:
                raise UnsupportedModel("non-integer hidden_state_dimension")
            p.hidden.append(h)
            p.features.append([(f.name, int(f.size)) for f in e.features])
        eidx = {n: i for i, n in enumerate(p.entities)}
        cell_of = {}
        for stage_name, mps in mi.get_mp_instances():
            for mp in mps:
                dst = mp.destination_entity
                upd = mp.update
                if upd.type != "recurrent_nn":
                    # GM:324-346 references an undefined `mp` (NameError): the reference cannot build it.
                    raise UnsupportedModel("feed-forward update is not executable in the reference (GM:338)")
                cell = upd.model
                if cell.type != "GRU":
                    raise UnsupportedModel("recurrent_type %s is not lowered (only GRU; LSTM passes one state, "
                                           "AUX:764)" % cell.type)
                options = _gru_options(cell.parameters)
                aggr = mp.aggregation.type
                if aggr not in ("sum", "ordered", "interleave", "concat", "attention", "convolution"):
                    raise UnsupportedModel("aggregation %r is not lowered yet" % aggr)
                act = 0
                if aggr == "convolution":       # AUX:370-374: activation_function, default relu
                    fn = getattr(mp.aggregation, "activation_function", "relu")
                    if fn not in _lib.ACT or fn in _lib.ACT_REFUSED_AT["convolution"]:
                        raise UnsupportedModel("activation %r not supported" % fn)
                    act = _lib.ACT[fn]
                feature_concat = aggr == "concat" and mp.aggregation.concat_axis == 2
                srcs = []
                nets = []
                din = None
                for s in mp.source_entities:
                    net = _message_net(s, dst, p, eidx)
                    nets.append(net)
                    slot = AdjSlot(s.adj_vector, s.name, dst)
                    if slot not in p.adj_slots:
                        p.adj_slots.append(slot)
                    il = -1
                    if aggr == "interleave":
                        key = "indices_" + s.name + "_to_" + dst
                        if key not in p.il_slots:
                            p.il_slots.append(key)
                        il = p.il_slots.index(key)
                    srcs.append((eidx[s.name], p.adj_slots.index(slot), il))
                    msg_dim = net["layers"][-1][1] if net else p.hidden[eidx[s.name]]
                    # axis-2 concat feeds the GRU the sources' concatenated messages (AUX:443-456)
                    din = (din or 0) + msg_dim if feature_concat else msg_dim
                if dst not in cell_of:
                    cell_of[dst] = len(p.cells)
                    p.cells.append((dst, din, p.hidden[eidx[dst]]))
                    p.cell_options.append(options)   # one cell per destination entity: its first MP's keys
                p.mps.append({"dst": eidx[dst], "aggr": aggr, "axis": getattr(mp.aggregation, "concat_axis", 0),
                              "cell": cell_of[dst], "sources": srcs, "stage": stage_name, "act": act,
                              "nets": nets})
                if aggr in ("attention", "convolution"):
                    # one weight set per model: the reference overwrites self.kernel1 / conv_kernel per
                    # MP and every MP uses the last one (GM:288-300)
                    setattr(p, aggr + "_dim", p.hidden[eidx[dst]])
        p._lower_readout(mi)
        return p

    @staticmethod
    def _dense_layers(arch, what, at="predict"):
        """(Dense layers, the other layers) of a readout stack.  The second list holds the stack's
        Dropout and LayerNormalization layers in the architecture's order, the one record of where
        each stands: ("dropout", before_layer, rate, seed) or ("layernorm", before_layer, epsilon,
        center, scale, name), before_layer = the Dense layer it precedes, len(layers) after the last
        one.  A Dropout is tf.nn.dropout in training and the identity otherwise; rate 0 is no layer, as
        TF returns x."""
        out, extra = [], []
        for l in arch.layers:
            if l.type == "Dropout":
                prm = dict(l.parameters)
                if set(prm) - {"rate", "name", "seed"}:
                    raise UnsupportedModel("Dropout options %s are not lowered" % sorted(set(prm) - {"rate", "name", "seed"}))
                if "rate" not in prm:
                    raise ValueError("Dropout: missing key 'rate'")
                rate = float(prm["rate"])
                if not 0.0 <= rate < 1.0:   # tf.nn.dropout raises ValueError
                    raise ValueError("Dropout rate must be in [0, 1), got %r" % rate)
                if rate > 0.0:
                    extra.append(("dropout", len(out), rate, int(prm.get("seed") or 0) & 0xFFFFFFFFFFFFFFFF))
                continue
            if l.type == "LayerNormalization":
                prm = dict(l.parameters)
                for k, v in prm.items():
                    if k in ("name", "epsilon", "center", "scale"):
                        continue
                    if k == "axis" and isinstance(v, (int, float)) and not isinstance(v, bool) and v == int(v):
                        if v not in (-1, 1):   # the stacks' tensors are [rows, units]
                            raise UnsupportedModel("LayerNormalization axis %d is not lowered (the last axis only: "
                                                   "-1 or 1)" % v)
                        continue
                    raise UnsupportedModel("LayerNormalization option '%s' is not lowered" % k)
                eps = float(prm.get("epsilon", 1e-3))
                if not eps >= 0.0:   # Keras raises ValueError
                    raise ValueError("LayerNormalization epsilon must be >= 0, got %r" % eps)
                extra.append(("layernorm", len(out), eps, bool(prm.get("center", True)), bool(prm.get("scale", True)),
                              prm.get("name")))
                continue
            if l.type != "Dense":
                raise UnsupportedModel("%s layer type %s is not lowered (Dense, Dropout and LayerNormalization only)"
                                       % (what, l.type))
            prm = dict(l.parameters)
            act = prm.get("activation", None)
            if act not in _lib.ACT or act in _lib.ACT_REFUSED_AT[at]:
                raise UnsupportedModel("activation %r not supported" % act)
            known = {"units", "activation", "kernel_regularizer", "name", "use_bias"}
            if set(prm) - known:
                raise UnsupportedModel("Dense options %s are not lowered" % sorted(set(prm) - known))
            out.append((prm.get("name"), int(prm["units"]), _lib.ACT[act], int(bool(prm.get("use_bias", True))),
                        float(prm.get("kernel_regularizer", 0.0) or 0.0)))
        for kind, label in (("dropout", "Dropout"), ("layernorm", "LayerNormalization")):
            if not out and any(e[0] == kind for e in extra):
                raise ValueError("%s network has a %s but no Dense layer" % (what, label))
        return out, extra

    def _lower_readout(self, mi):
        """The readout list (GM:605-655) up to the first predict, which returns (GM:629); names
        resolve like get_global_var_or_input (GM:660-675): entity states, then op outputs, later
        outputs shadowing earlier names."""
        names = {n: i for i, n in enumerate(self.entities)}
        self.ro_widths = list(self.hidden)
        self.ro_spaces = [("entity", i) for i in range(len(self.entities))]

        def resolve(name):
            if name not in names:
                raise UnsupportedModel("readout input %r is not an entity state or a readout output (raw input "
                                       "features are not lowered as readout inputs)" % name)
            return names[name]

        def add(name, width, space):
            names[name] = len(self.ro_widths)
            self.ro_widths.append(width)
            self.ro_spaces.append(space)

        pred = None
        for counter, op in enumerate(mi.get_readout_operations()):
            if op.type == "predict":
                pred = (counter, op)
                break
            ids = [resolve(n) for n in op.input]
            first = self.ro_spaces[ids[0]]
            d = {"type": op.type, "inputs": ids, "mode": 0, "adj": -1, "layers": [], "counter": counter}
            if op.type == "neural_network":
                d["layers"], d["extra"] = self._dense_layers(op.architecture, "readout", "readout_op")
                d["in_width"] = sum(self.ro_widths[i] for i in ids)
                add(op.output_name, d["layers"][-1][1], first)
            elif op.type == "pooling":
                if op.type_pooling not in _lib.POOLING:
                    raise UnsupportedModel("pooling type %r is not lowered" % op.type_pooling)
                d["mode"] = _lib.POOLING[op.type_pooling]
                add(op.output_name, self.ro_widths[ids[0]], ("graph",))
            elif op.type == "product":
                if op.type_product != "element_wise":
                    raise UnsupportedModel("product %r is not lowered: tf.tensordot(axes=0) is a rank-4 outer product "
                                           "that the reference records as width 1 (GM:374-375)" % op.type_product)
                if len(ids) < 2:
                    raise UnsupportedModel("product needs two inputs")
                space = first if first != ("graph",) else self.ro_spaces[ids[1]]
                add(op.output_name, self.ro_widths[ids[0]], space)
            elif op.type == "extend_adjacencies":
                slots = [k for k, sl in enumerate(self.adj_slots) if sl.adj == op.adj_list]
                if not slots:
                    raise UnsupportedModel("extend_adjacencies: adjacency %r is not read by any message passing "
                                           "(the reference's input has no src_/dst_ for it)" % op.adj_list)
                d["adj"] = slots[0]
                add(op.output_name[0], self.ro_widths[ids[0]], ("adj", slots[0]))
                add(op.output_name[1], self.ro_widths[ids[1]], ("adj", slots[0]))
            else:
                raise UnsupportedModel("readout operation %r is not lowered" % op.type)
            self.readout_ops.append(d)
        if pred is None:
            raise UnsupportedModel("the readout has no predict operation")
        self.predict_counter, op = pred
        self.readout_label = op.label
        self.readout_inputs = [resolve(n) for n in op.input]
        self.dense, self.extra = self._dense_layers(op.architecture, "readout")

    @property
    def predict_space(self):
        return self.ro_spaces[self.readout_inputs[0]]

    def _stacks(self):
        """[(stack, input width, Dense layers, the other layers)]: the readout operations in order (only
        a neural_network has layers), then predict (stack -1)."""
        out = [(k, op.get("in_width", 0), op["layers"], op.get("extra", [])) for k, op in enumerate(self.readout_ops)]
        return out + [(-1, sum(self.ro_widths[i] for i in self.readout_inputs), self.dense, self.extra)]

    def _sites(self, kind):
        """[(stack, fan, Dense layers, order, record)] of the layers of one kind in the engine's site
        order: stacks as _stacks, and within a stack as listed, which is by position.  order = the
        layer's place among the layers of both kinds in front of the same Dense layer."""
        return [(stack, fan, layers, sum(f[1] == e[1] for f in extra[:i]), e)
                for stack, fan, layers, extra in self._stacks() for i, e in enumerate(extra) if e[0] == kind]

    def dropout_sites(self):
        """[(site, stack, before_layer, rate, seed)] in site order: readout operations in order, then
        predict (stack -1), by position within a stack (ign_plan_add_dropout)."""
        return [(site, r[0]) + r[4][1:] for site, r in enumerate(self._sites("dropout"))]

    def layernorm_sites(self):
        """[(site, stack, before_layer, order, epsilon, center, scale, units, name)] in the engine's order
        (ign_plan_add_layernorm): stacks as dropout_sites, by position within a stack.  units = the
        width it normalises: the input width of the Dense layer it precedes, or the stack's output width."""
        return [(site, stack, before, order, eps, center, scale, layers[before - 1][1] if before else fan, name)
                for site, (stack, fan, layers, order, (_, before, eps, center, scale, name))
                in enumerate(self._sites("layernorm"))]

    def stack_sites(self):
        """The ign_plan_add_dropout / ign_plan_add_layernorm calls that build the plan's layers, each
        stack's in the architecture's order: [("dropout", stack, before, rate, seed) |
        ("layernorm", stack, before, epsilon, center, scale)]."""
        return [(e[0], stack) + (e[1:] if e[0] == "dropout" else (e[1], e[2], int(e[3]), int(e[4])))
                for stack, _, _, extra in self._stacks() for e in extra]

    def dead_in_last_iter(self):
        """Per MP, in execution order: True where nothing reads what its last iteration's update writes
        (ign_plan_mp_dead_last), so the graph-resident forward leaves that update out until Batch.state asks for the
        entity.  Lowered on the host: needs no GPU."""
        desc, keep = self.to_desc()
        h = C.c_void_p()
        check(lib.ign_plan_create(C.byref(desc), 0, C.byref(h)))
        try:
            self.set_cell_options(h)
            dead = C.c_int32()
            out = []
            for mi in range(len(self.mps)):
                check(lib.ign_plan_mp_dead_last(h, mi, C.byref(dead)))
                out.append(bool(dead.value))
            return out
        finally:
            lib.ign_plan_destroy(h)

    def set_cell_options(self, handle):
        """The cells' options on a plan just created from ``to_desc`` (ign_plan_set_cell_options; ign_cell_desc
        has no room for them).  A cell of Keras defaults needs no call."""
        for c, opt in enumerate(self.cell_options):
            if opt != _gru_options({}):
                o = _lib.CellOptions(*[int(v) for v in opt])
                check(lib.ign_plan_set_cell_options(handle, c, C.byref(o)))

    # ------------------------------------------------------------------ C structures
    def to_desc(self):
        keep = []
        ents = (_lib.EntityDesc * len(self.entities))(
            *[_lib.EntityDesc(h, sum(s for _, s in f)) for h, f in zip(self.hidden, self.features)])
        mps = (_lib.MPDesc * len(self.mps))()
        for i, m in enumerate(self.mps):
            srcs = (_lib.SourceDesc * len(m["sources"]))()
            for k, src in enumerate(m["sources"]):
                net = m.get("nets", [None] * len(m["sources"]))[k]
                if net:
                    ins = (C.c_int32 * len(net["inputs"]))(*[_lib.MSG_INPUT[x] for x in net["inputs"]])
                    lay = (_lib.DenseDesc * len(net["layers"]))(*[_lib.DenseDesc(u, a, b, l2)
                                                                  for _, u, a, b, l2 in net["layers"]])
                    keep += [ins, lay]
                    srcs[k] = _lib.SourceDesc(*src, len(net["inputs"]), ins, net["param_dim"], len(net["layers"]), lay)
                else:
                    srcs[k] = _lib.SourceDesc(*src)
            keep.append(srcs)
            mps[i] = _lib.MPDesc(m["dst"], _lib.AGGR[m["aggr"]], int(m["axis"] or 0), m["cell"], len(m["sources"]),
                                 C.cast(srcs, C.POINTER(_lib.SourceDesc)), int(m.get("act", 0)))
        cells = (_lib.CellDesc * len(self.cells))(*[_lib.CellDesc(din, h) for _, din, h in self.cells])
        ro = (C.c_int32 * len(self.readout_inputs))(*self.readout_inputs)
        dense = (_lib.DenseDesc * len(self.dense))(*[_lib.DenseDesc(u, a, b, l2) for _, u, a, b, l2 in self.dense])
        rops = (_lib.ReadoutOpDesc * max(1, len(self.readout_ops)))()
        for k, op in enumerate(self.readout_ops):
            ins = (C.c_int32 * len(op["inputs"]))(*op["inputs"])
            lay = (_lib.DenseDesc * max(1, len(op["layers"])))(*[_lib.DenseDesc(u, a, b, l2)
                                                                 for _, u, a, b, l2 in op["layers"]])
            keep += [ins, lay]
            rops[k] = _lib.ReadoutOpDesc(_lib.READOUT_OP[op["type"]], len(op["inputs"]), ins, op["mode"], op["adj"],
                                         len(op["layers"]), lay)
        keep += [ents, mps, cells, ro, dense, rops]
        d = _lib.PlanDesc(self.iterations, len(self.entities), ents, len(self.adj_slots), len(self.il_slots),
                          len(self.mps), mps, len(self.cells), cells, len(self.readout_inputs), ro,
                          len(self.dense), dense, len(self.readout_ops), rops)
        return d, keep

    # ------------------------------------------------------------------ parameters
    def param_specs(self):
        """[(name, shape)] in the engine's tensor order (ign_plan_param_tensor)."""
        specs = []
        for (dst, din, h), (_, _, use_bias, reset_after) in zip(self.cells, self.cell_options):
            specs += [(dst + "_update/kernel", (din, 3 * h)), (dst + "_update/recurrent_kernel", (h, 3 * h))]
            if use_bias:   # Keras' GRUCell: [2][3H]; reset_after false, [3H]; use_bias false, no variable
                specs.append((dst + "_update/bias", (2, 3 * h) if reset_after else (3 * h,)))
        for m in self.mps:
            for net in m.get("nets", []):
                if not net:
                    continue
                fan = net["din"]
                for name, units, _, use_bias, _ in net["layers"]:
                    specs.append((net["prefix"] + name + "/kernel", (fan, units)))
                    if use_bias:
                        specs.append((net["prefix"] + name + "/bias", (units,)))
                    fan = units
        if self.convolution_dim:
            F = self.convolution_dim
            specs.append(("convolution/kernel", (F, F)))
        if self.attention_dim:
            F = self.attention_dim
            specs += [("attention/kernel1", (F, F)), ("attention/kernel2", (F, F)), ("attention/attn_kernel", (2 * F, 1))]
        def stack(counter, fan_in, layers, extra):
            # a LayerNormalization's gamma / beta stand in front of the Dense layer it precedes
            for li in range(len(layers) + 1):
                for e in extra:
                    if e[0] == "layernorm" and e[1] == li:
                        pre = "readout_model_%d/%s" % (counter, e[5])
                        specs.extend([(pre + "/gamma", (fan_in,))] * e[4] + [(pre + "/beta", (fan_in,))] * e[3])
                if li == len(layers):
                    break
                name, units, _, use_bias, _ = layers[li]
                pre = "readout_model_%d/%s" % (counter, name or ("layer_%d" % li))
                specs.append((pre + "/kernel", (fan_in, units)))
                if use_bias:
                    specs.append((pre + "/bias", (units,)))
                fan_in = units

        for op in self.readout_ops:
            stack(op["counter"], op.get("in_width", 0), op["layers"], op.get("extra", []))
        stack(self.predict_counter, sum(self.ro_widths[i] for i in self.readout_inputs), self.dense, self.extra)
        return specs

    def init_params(self, seed: int = 0, bias_scale: float = 0.0) -> dict:
        """Keras default initialisers: glorot_uniform kernels, orthogonal recurrent kernels, zero
        biases, LayerNormalization gamma ones and beta zeros (``bias_scale`` > 0 draws biases and
        beta uniformly instead, and gamma around one, for tests)."""
        rng = np.random.default_rng(seed)
        out = {}
        for name, shape in self.param_specs():
            if name.endswith("recurrent_kernel"):
                a = rng.standard_normal((shape[1], shape[0]))
                q, r = np.linalg.qr(a)
                q = q * np.sign(np.diag(r))
                out[name] = q.T.astype(np.float32)
            elif name.endswith("kernel") or name.endswith("kernel1") or name.endswith("kernel2"):
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                out[name] = rng.uniform(-lim, lim, shape).astype(np.float32)
            elif name.endswith("/gamma"):
                out[name] = ((1.0 + rng.uniform(-bias_scale, bias_scale, shape)).astype(np.float32) if bias_scale
                             else np.ones(shape, np.float32))
            else:
                out[name] = (rng.uniform(-bias_scale, bias_scale, shape).astype(np.float32) if bias_scale
                             else np.zeros(shape, np.float32))
        return out


class Engine:
    """A plan on one device (``ign_plan``)."""

    def __init__(self, plan: MPPlan, device: int = 0):
        self.plan = plan
        self.device = device
        desc, self._keep = plan.to_desc()
        h = C.c_void_p()
        check(lib.ign_plan_create(C.byref(desc), device, C.byref(h)))
        self.handle = h
        plan.set_cell_options(h)
        for kind, *args in plan.stack_sites():   # ign_dense_desc has no room for them
            check((lib.ign_plan_add_dropout if kind == "dropout" else lib.ign_plan_add_layernorm)(h, *args))
        self.params_version = 0   # bumped by every parameter update (SplitBatch re-syncs its replicas)
        self._replicas = []
        _LIVE_ENGINES.add(self)
        n = C.c_int64()
        check(lib.ign_plan_num_params(h, C.byref(n)))
        self.n_params = n.value
        nt = C.c_int32()
        check(lib.ign_plan_num_param_tensors(h, C.byref(nt)))
        self.layout = []
        specs = plan.param_specs()
        if nt.value != len(specs):
            raise RuntimeError("parameter layout mismatch between host and engine")
        for i in range(nt.value):
            kind, owner, off, rows, cols = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
            check(lib.ign_plan_param_tensor(h, i, C.byref(kind), C.byref(owner), C.byref(off), C.byref(rows),
                                            C.byref(cols)))
            name, shape = specs[i]
            if int(np.prod(shape)) != rows.value * cols.value:
                raise RuntimeError("parameter %s: engine shape %dx%d vs host %s" % (name, rows.value, cols.value, shape))
            self.layout.append((name, shape, off.value))

    def set_params(self, params: dict):
        """Every tensor of the layout, by its Keras-like name and with its exact shape (the
        reference's Saver.restore also refuses a missing variable or a shape mismatch)."""
        flat = np.zeros(self.n_params, np.float32)
        missing = [name for name, _, _ in self.layout if name not in params]
        if missing:
            raise ValueError("set_params: missing parameter tensor(s) %s" % ", ".join(missing))
        for name, shape, off in self.layout:
            v = np.asarray(params[name], dtype=np.float32)
            if v.size != int(np.prod(shape)) or (v.ndim > 1 and tuple(v.shape) != tuple(shape)):
                raise ValueError("set_params: %s has shape %s, the model needs %s" % (name, tuple(v.shape), tuple(shape)))
            v = np.ascontiguousarray(v).reshape(-1)
            flat[off:off + v.size] = v
        check(lib.ign_plan_set_params(self.handle, flat.ctypes.data_as(C.c_void_p), 0))
        self.params_version += 1

    def set_timing(self, on: bool, kinds=None):
        """Per-launch HIP event timing (resets the statistics); ``kinds``: kernel kind names to
        instrument (default all)."""
        check(lib.ign_plan_set_timing(self.handle, int(on)))
        mask = 0xFFFFFFFF if kinds is None else sum(1 << _lib.KERNEL_KINDS.index(k) for k in kinds)
        check(lib.ign_plan_set_timing_kinds(self.handle, mask))

    def stats(self) -> dict:
        s = _lib.Stats()
        check(lib.ign_stats(self.handle, C.byref(s)))
        return {k: {"launches": s.launches[i], "ms": s.ms[i], "flops": s.flops[i], "bytes": s.bytes[i],
                    "mfma_bf16": s.mfma_bf16[i], "mfma_f32": s.mfma_f32[i]}
                for i, k in enumerate(_lib.KERNEL_KINDS)}

    def synchronize(self):
        check(lib.ign_synchronize(self.handle))

    def trim_cache(self):
        """Release the idle cached device blocks of this plan and the idle pinned host blocks
        (ign_plan_trim_cache), e.g. when torch or RCCL run short of memory."""
        check(lib.ign_plan_trim_cache(self.handle))

    def set_stream(self, hip_stream: int):
        """Run on an external HIP stream (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        check(lib.ign_plan_set_stream(self.handle, C.c_void_p(hip_stream)))

    # ---- training (ignnition_amd.training drives these) --------------------------
    def get_params(self) -> dict:
        flat = np.empty(self.n_params, np.float32)
        check(lib.ign_plan_get_params(self.handle, flat.ctypes.data_as(C.c_void_p)))
        return {name: flat[off:off + int(np.prod(shape))].reshape(shape).copy() for name, shape, off in self.layout}

    def loss(self, kind: int, pred, labels, dpred, want_loss: bool = True) -> float:
        """The lowered Keras loss of ``kind`` (ign_loss_kind of its name).  Device tensors or addresses:
        pred/labels/dpred [n] fp32 (n = labels.numel()).  Returns the loss; writes dLoss/dpred."""
        out = C.c_double()
        check(lib.ign_loss(self.handle, int(kind), _ptr(pred), _ptr(labels), labels.numel(), _ptr(dpred),
                           C.byref(out) if want_loss else None))
        return out.value if want_loss else None

    def mse_loss(self, pred, labels, dpred, want_loss: bool = True) -> float:
        return self.loss(0, pred, labels, dpred, want_loss)

    def l2_loss(self) -> float:
        out = C.c_double()
        check(lib.ign_l2_loss(self.handle, C.byref(out)))
        return out.value

    def optimizer_step(self, desc, grads, slots, iteration: int, lr: float):
        """One update of the lowered Keras optimizer ``desc`` (an ``_lib.OptimizerDesc``); ``slots``: its
        ign_optimizer_num_slots device buffers of n_params floats, in that call's order."""
        arr = (C.c_void_p * max(1, len(slots)))(*[_ptr(s) for s in slots])
        check(lib.ign_optimizer_step(self.handle, C.byref(desc), _ptr(grads), arr, len(slots), int(iteration), lr))
        self.params_version += 1

    def nonfinite_count(self, tensor, counter):
        """ign_nonfinite_count: enqueue, on the plan's stream, ``counter += the number of NaN / +-Inf
        values of tensor`` (a contiguous float32 device tensor, any 4-byte-aligned view of one; counter:
        one 4-byte integer on the device, read as unsigned).  No host wait; an empty tensor launches nothing."""
        if str(tensor.dtype) != "torch.float32" or not tensor.is_contiguous():
            raise ValueError("nonfinite_count: the tensor must be contiguous float32, not %s" % (tensor.dtype,))
        if counter.element_size() != 4 or counter.numel() != 1 or counter.is_floating_point():
            raise ValueError("nonfinite_count: the counter must be one 4-byte integer")
        if tensor.numel():   # (an empty tensor may have no address)
            check(lib.ign_nonfinite_count(self.handle, _ptr(tensor), tensor.numel(), _ptr(counter)))

    def adam_step(self, grads, m, v, iteration: int, lr: float, beta1=0.9, beta2=0.999, epsilon=1e-7):
        """ign_adam_step: ``optimizer_step`` for Adam with loose hyper-parameters."""
        check(lib.ign_adam_step(self.handle, _ptr(grads), _ptr(m), _ptr(v), int(iteration), lr, beta1, beta2, epsilon))
        self.params_version += 1

    def replicas(self, n: int) -> list:
        """``n`` more plans of this model on this device (each its own HIP stream), created once and
        kept; their parameters follow this engine's (SplitBatch re-syncs them when they changed)."""
        while len(self._replicas) < n:
            r = Engine(self.plan, self.device)
            r._synced = -1
            self._replicas.append(r)
        for r in self._replicas[:n]:
            if r._synced != self.params_version:
                flat = np.empty(self.n_params, np.float32)
                check(lib.ign_plan_get_params(self.handle, flat.ctypes.data_as(C.c_void_p)))
                check(lib.ign_plan_set_params(r.handle, flat.ctypes.data_as(C.c_void_p), 0))
                r._synced = self.params_version
        return self._replicas[:n]

    def gather_rows(self, src, idx, dst):
        """dst[i] = src[idx[i]] (device tensors: src [R, C] fp32, idx [n] int32, dst [n, C])."""
        n = idx.numel()
        cols = src.shape[1]
        check(lib.ign_gather_rows(self.handle, C.c_void_p(src.data_ptr()), src.stride(0), C.c_void_p(idx.data_ptr()),
                                  n, cols, C.c_void_p(dst.data_ptr())))

    def close(self):
        # ign_batch_destroy reads its plan (stream, block cache): while a batch of this engine is
        # open, the plan stays, and the last batch's close() destroys it.  (The collector finalises
        # an engine and its batches in no particular order when they die in one reference cycle,
        # e.g. in the traceback of a failed test.)
        if getattr(self, "_open_batches", 0) > 0:
            self._close_pending = True
            return
        for r in getattr(self, "_replicas", []):
            r.close()
        self._replicas = []
        h = getattr(self, "handle", None)
        if h:
            lib.ign_plan_destroy(h)
            self.handle = None

    def __del__(self):
        self.close()


def _ptr(x) -> C.c_void_p:
    """Device pointer of a torch tensor, or a raw integer address."""
    return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1))


class BatchedGraphs:
    """A batch of graphs as graph-concatenated arrays: key -> (values, per-graph lengths), the
    keys of the input_fn dict (GM:127-158).  ``num_<entity>`` holds one value per graph."""

    def __init__(self, arrays: dict, num_graphs: int):
        self.arrays = arrays
        self.num_graphs = num_graphs

    @classmethod
    def from_dicts(cls, graphs: list) -> "BatchedGraphs":
        keys = {}
        for x in graphs:
            for k in x:
                keys.setdefault(k, None)
        arrays = {}
        for k in keys:
            if not all(k in x for x in graphs):
                continue
            parts = [np.asarray(x[k]).reshape(-1) for x in graphs]
            arrays[k] = (np.concatenate(parts) if parts else np.zeros(0), np.array([len(v) for v in parts], np.int64))
        return cls(arrays, len(graphs))

    def get(self, key):
        if key not in self.arrays:
            raise KeyError("batch has no array %r" % key)
        return self.arrays[key]

    def __contains__(self, key):
        return key in self.arrays


def batch_desc(p: "MPPlan", graphs, halo_rows: dict = None):
    """The ``ign_batch_desc`` of a list of feature dicts or a ``BatchedGraphs`` for plan ``p``:
    (desc, arrays the desc points into, (G, E, num [G, E], edge counts [G, A], halo or None))."""
    bg = graphs if isinstance(graphs, BatchedGraphs) else BatchedGraphs.from_dicts(graphs)
    G = bg.num_graphs
    E = len(p.entities)
    num = np.zeros((G, E), np.int64)
    for e, name in enumerate(p.entities):
        v, _ = bg.get("num_" + name)
        num[:, e] = np.asarray(v, np.int64).reshape(G)
    feats = []
    for e, name in enumerate(p.entities):
        cols = []
        for fname, size in p.features[e]:
            v, lens = bg.get(fname)
            if not np.array_equal(np.asarray(lens, np.int64), num[:, e] * size):
                raise ValueError("feature %s: %s values per graph for %s nodes of size %d"
                                 % (fname, list(lens), list(num[:, e]), size))
            cols.append(np.asarray(v, np.float32).reshape(-1, size))
        feats.append(np.ascontiguousarray(np.concatenate(cols, 1)) if cols else None)
    A = len(p.adj_slots)
    cnt = np.zeros((G, A), np.int64)
    srcs, dsts, seqs = [], [], []
    for a, slot in enumerate(p.adj_slots):
        ks, kd, kq = slot.keys
        (s, ls), (d, ld), (q, lq) = bg.get(ks), bg.get(kd), bg.get(kq)
        if not (np.array_equal(ls, ld) and np.array_equal(ls, lq)):
            raise ValueError("%s/%s/%s have different lengths" % (ks, kd, kq))
        cnt[:, a] = ls
        srcs.append(s), dsts.append(d), seqs.append(q)
    I = len(p.il_slots)
    il_len = np.zeros((G, max(I, 1)), np.int64)
    ils = []
    for i, key in enumerate(p.il_slots):
        v, lens = bg.get(key)
        il_len[:, i] = lens
        ils.append(v)
    # index arrays: int32 as they come when every one is (the native reader's narrow gather,
    # index_bytes = 4: no widening copy here, half the bytes the build reads), else all as int64
    narrow = all(np.asarray(x).dtype == np.int32 for x in srcs + dsts + seqs + ils)
    conv = (lambda x: np.ascontiguousarray(np.asarray(x).reshape(-1))) if narrow else _i64
    srcs, dsts, seqs, ils = ([conv(x) for x in l] for l in (srcs, dsts, seqs, ils))
    fp = C.POINTER(C.c_float)
    lp = C.POINTER(C.c_int64)
    feat_ptrs = (fp * E)(*[f.ctypes.data_as(fp) if f is not None and f.size else fp() for f in feats])
    mk = lambda arrs: (lp * max(len(arrs), 1))(*[C.cast(a.ctypes.data, lp) for a in arrs])
    prm_arrays = []
    for slot in p.adj_slots:
        key = "params_" + slot.adj
        prm_arrays.append(np.ascontiguousarray(np.asarray(bg.get(key)[0], np.float32)) if key in bg else None)
    halo = None
    if halo_rows:
        halo = np.array([int(halo_rows.get(name, 0)) for name in p.entities], np.int64)
    ptrs = (feat_ptrs, mk(srcs), mk(dsts), mk(seqs), mk(ils), (fp * max(A, 1))(*[a.ctypes.data_as(fp) if a is not None
                                                                                 else fp() for a in prm_arrays]))
    desc = _lib.BatchDesc(G, num.ctypes.data_as(lp), ptrs[0], cnt.ctypes.data_as(lp), ptrs[1], ptrs[2], ptrs[3],
                          il_len.ctypes.data_as(lp), ptrs[4], halo.ctypes.data_as(lp) if halo is not None else lp(),
                          ptrs[5], 4 if narrow else 8)
    keep = (num, feats, cnt, srcs, dsts, seqs, il_len, ils, prm_arrays, halo, ptrs)
    return desc, keep, (G, E, num, cnt, halo)


def feature_rows(features, rows: int, values) -> np.ndarray:
    """The ``[rows, F]`` float32 array ``Batch.set_features`` hands to the engine, without a GPU.
    ``features``: the entity's ``[(name, size)]`` of ``MPPlan.features`` (F = the sum of the sizes);
    ``values``: a ``{feature name: array}`` dict, each array holding ``rows * size`` values (``[rows]``
    for size 1, ``[rows, size]`` or flat), laid side by side in the plan's column order; or one array
    of ``rows * F`` values, ``[rows, F]`` or flat.  A missing or unknown name, or an array of another
    size, is a ``ValueError``."""
    F = sum(size for _, size in features)
    if F == 0:
        raise ValueError("the entity has no features")
    if isinstance(values, dict):
        names = [name for name, _ in features]
        missing = [n for n in names if n not in values]
        unknown = sorted(set(values) - set(names))
        if missing or unknown:
            raise ValueError("set_features: missing feature(s) %s, unknown feature(s) %s (the entity has %s)"
                             % (missing, unknown, names))
        cols = []
        for name, size in features:
            v = np.asarray(values[name], np.float32)
            if v.size != rows * size or (v.ndim == 2 and v.shape != (rows, size)) or v.ndim > 2:
                raise ValueError("set_features: feature %s has shape %s, the batch needs %d rows of width %d"
                                 % (name, tuple(v.shape), rows, size))
            cols.append(v.reshape(rows, size))
        return np.ascontiguousarray(np.concatenate(cols, 1))
    v = np.asarray(values, np.float32)
    if v.size != rows * F or (v.ndim == 2 and v.shape != (rows, F)) or v.ndim > 2:
        raise ValueError("set_features: values have shape %s, the batch needs %d rows of width %d"
                         % (tuple(v.shape), rows, F))
    return np.ascontiguousarray(v.reshape(rows, F))


def edge_param_sources(plan, adj: str):
    """``(param_dim, [(mp, source, adjacency slot)])``: the MP sources whose message network reads the
    per-edge parameters of adjacency ``adj`` (``params_<adj>``) as ``edge_params``, in plan order; each
    owns one buffer in a batch.  ``ValueError`` when there is none.  No GPU is touched."""
    found = []
    for m, mp in enumerate(plan.mps):
        for k, (src, net) in enumerate(zip(mp["sources"], mp.get("nets", []))):
            if net and "edge_params" in net["inputs"] and plan.adj_slots[src[1]].adj == adj:
                found.append((m, k, src[1], int(net["param_dim"])))
    if not found:
        reads = sorted({plan.adj_slots[src[1]].adj for mp in plan.mps
                        for src, net in zip(mp["sources"], mp.get("nets", [])) if net and "edge_params" in net["inputs"]})
        raise ValueError("no message network reads the edge parameters of adjacency %r (read: %s)" % (adj, reads))
    return found[0][3], [f[:3] for f in found]


def edge_param_rows(n_edges: int, param_dim: int, values, what: str = "set_edge_params") -> np.ndarray:
    """The ``[n_edges, param_dim]`` float32 array ``Batch.set_edge_params`` hands to the engine, without
    a GPU: ``values`` as ``[n_edges, param_dim]`` or flat (``[n_edges]`` for one parameter), in the
    order of the ``params_<adj>`` the batch was built from.  Another size or shape is a ``ValueError``."""
    v = np.asarray(values, np.float32)
    if v.size != n_edges * param_dim or (v.ndim == 2 and v.shape != (n_edges, param_dim)) or v.ndim > 2:
        raise ValueError("%s: values have shape %s, the batch needs %d rows of width %d"
                         % (what, tuple(v.shape), n_edges, param_dim))
    return np.ascontiguousarray(v.reshape(n_edges, param_dim))


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _device_rows(x, rows: int, F: int, what: str):
    """A CUDA tensor as [rows, F] contiguous float32 rows, or ValueError."""
    import torch
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("%s: a contiguous float32 CUDA tensor is needed" % what)
    if x.numel() != rows * F or (x.dim() == 2 and tuple(x.shape) != (rows, F)) or x.dim() > 2:
        raise ValueError("%s: tensor has shape %s, the batch needs %d rows of width %d"
                         % (what, tuple(x.shape), rows, F))
    return x


class Batch:
    """A disjoint-union batch of graphs on the device (``ign_batch``).

    ``graphs``: list of feature dicts with the input_fn keys (GM:127-158), features already
    normalised.  Graph-local indices are kept; the engine offsets them per graph."""

    def __init__(self, engine: Engine, graphs, halo_rows: dict = None):
        """``graphs``: a list of feature dicts, or a ``BatchedGraphs`` (graph-concatenated arrays,
        e.g. from the native dataset reader).  ``halo_rows``: {entity: extra rows} for one
        edge-cut partition (see partition.py)."""
        p = engine.plan
        self.engine = engine
        desc, keep, (G, E, num, cnt, halo) = batch_desc(p, graphs, halo_rows)
        self._arrays = keep                 # (may view the caller's buffers) until the engine copied them
        self.halo = [0] * E if halo is None else [int(v) for v in halo]
        h = C.c_void_p()
        check(lib.ign_batch_create(engine.handle, C.byref(desc), C.byref(h)))
        self.handle = h
        engine._open_batches = getattr(engine, "_open_batches", 0) + 1
        _LIVE_BATCHES.add(self)
        info = _lib.BatchInfo()
        check(lib.ign_batch_info(h, C.byref(info)))
        self.num_graphs = info.num_graphs
        self.predictions = info.predictions
        self.output_units = info.output_units
        self.edges_per_forward = info.edges_per_forward
        self.gru_steps_per_forward = info.gru_steps_per_forward
        self.rows = list(info.rows)[:E]
        self.graph_rows = num
        self.graph_edges = cnt               # [graphs, adjacency slots]
        space = p.predict_space     # rows of the predict input space per graph (GM:716-724 splits)
        if space[0] == "entity":
            self.graph_predictions = num[:, space[1]].copy()
        elif space[0] == "graph":
            self.graph_predictions = np.ones(G, np.int64)
        else:
            self.graph_predictions = cnt[:, space[1]].copy()
        self._arrays = None  # the engine copied what it needs
        self._bound = {}

    # ---- stepped forward (edge-cut partitions) -----------------------------------
    def begin(self):
        check(lib.ign_forward_begin(self.engine.handle, self.handle))

    def run_mp(self, mp: int, part: str = "all"):
        check(lib.ign_forward_mp(self.engine.handle, self.handle, mp, _lib.PART[part]))

    def end(self, to_host: bool = True):
        out = np.empty((self.predictions, self.output_units), np.float32) if to_host else None
        check(lib.ign_forward_end(self.engine.handle, self.handle,
                                  out.ctypes.data_as(C.c_void_p) if to_host else None))
        return out

    def mp_split(self, mp: int):
        """(interior, boundary) destination counts of MP ``mp``."""
        a, b = C.c_int64(), C.c_int64()
        check(lib.ign_batch_mp_split(self.handle, mp, C.byref(a), C.byref(b)))
        return a.value, b.value

    def bind_state(self, entity: str, buf0, buf1):
        """Use two caller-owned device buffers (torch tensors) as the entity's state buffers."""
        e = self.engine.plan.entities.index(entity)
        cap = min(buf0.numel(), buf1.numel())
        check(lib.ign_batch_bind_state(self.engine.handle, self.handle, e, C.c_void_p(buf0.data_ptr()),
                                       C.c_void_p(buf1.data_ptr()), cap))
        self._bound[entity] = (buf0, buf1)

    # ---- what-if analysis: new feature values on the same graphs, and their gradient -----------
    def _feature_entity(self, entity: str):
        p = self.engine.plan
        if entity not in p.entities:
            raise ValueError("no entity %r (the model has %s)" % (entity, p.entities))
        e = p.entities.index(entity)
        return e, self.rows[e], sum(size for _, size in p.features[e])

    def set_features(self, entity: str, values):
        """Replace the entity's feature values in place (ign_batch_set_features): from the next forward
        on, the batch computes what a fresh batch built with these values computes, bit for bit.
        ``values``: a ``{feature name: array}`` dict or one ``[rows, F]`` array (``feature_rows``),
        normalised as the values the batch was built from; or a contiguous float32 CUDA tensor of
        ``[rows, F]``, read by its pointer in the engine's stream order with no host copy (make the
        engine's stream wait for whatever wrote it).  Refused between a training forward and the end
        of its backward, and on an edge-cut partition."""
        e, rows, F = self._feature_entity(entity)
        if F == 0:   # the engine's refusal and its text
            values = np.zeros(1, np.float32)
            check(lib.ign_batch_set_features(self.engine.handle, self.handle, e, values.ctypes.data_as(C.c_void_p)))
        if _is_device_tensor(values):
            src = _device_rows(values, rows, F, "set_features")
        else:
            src = feature_rows(self.engine.plan.features[e], rows, values)   # (the engine waits for a host copy)
        ptr = C.c_void_p(src.data_ptr()) if _is_device_tensor(values) else src.ctypes.data_as(C.c_void_p)
        check(lib.ign_batch_set_features(self.engine.handle, self.handle, e, ptr))

    def feature_gradients(self, entity: str, out=None):
        """dLoss/d(feature values) of the entity after a completed backward (ign_batch_feature_gradients),
        for the loss whose ``dpred`` that backward was given: ``{feature name: ndarray [rows, size]}``.
        With ``out`` a contiguous float32 CUDA tensor ``[rows, F]`` it is filled in the engine's stream
        order, with no host copy or wait, and returned."""
        import torch
        e, rows, F = self._feature_entity(entity)
        if out is not None:
            if not _is_device_tensor(out):
                raise ValueError("feature_gradients: out must be a CUDA tensor")
            _device_rows(out, rows, F, "feature_gradients")
            check(lib.ign_batch_feature_gradients(self.engine.handle, self.handle, e, C.c_void_p(out.data_ptr())))
            return out
        buf = torch.empty((rows, max(F, 1)), dtype=torch.float32, device="cuda:%d" % self.engine.device)
        check(lib.ign_batch_feature_gradients(self.engine.handle, self.handle, e, C.c_void_p(buf.data_ptr())))
        self.engine.synchronize()
        g = buf.cpu().numpy()
        res, col = {}, 0
        for name, size in self.engine.plan.features[e]:
            res[name] = g[:, col:col + size].copy()
            col += size
        return res

    # ---- what-if analysis: new per-edge parameters (params_<adj>) on the same graphs, their gradient
    def _edge_sources(self, adj: str):
        """(edges of the batch, param_dim, [(mp, source)]) of adjacency ``adj`` (edge_param_sources)."""
        P, found = edge_param_sources(self.engine.plan, adj)
        return int(self.graph_edges[:, found[0][2]].sum()), P, [(m, k) for m, k, _ in found]

    def set_edge_params(self, adj: str, values):
        """Replace the per-edge parameters of adjacency ``adj`` in place (ign_batch_set_edge_params, on
        every MP source whose message network reads them): from the next forward on, the batch computes
        what a fresh batch built with these ``params_<adj>`` computes, bit for bit.  ``values``:
        ``[n_edges, param_dim]`` in the batch's edge order (the graphs' ``params_<adj>`` stacked), as an
        array or as a contiguous float32 CUDA tensor, which is read by its pointer in the engine's
        stream order with no host copy (make the engine's stream wait for whatever wrote it).  Refused
        between a training forward and the end of its backward."""
        ne, P, sources = self._edge_sources(adj)
        if _is_device_tensor(values):
            ptr = C.c_void_p(_device_rows(values, ne, P, "set_edge_params").data_ptr())
        else:
            src = edge_param_rows(ne, P, values)   # (the engine waits for a host copy)
            ptr = src.ctypes.data_as(C.c_void_p)
        if ne == 0:   # (an empty tensor has no address to hand over)
            return
        for m, k in sources:
            check(lib.ign_batch_set_edge_params(self.engine.handle, self.handle, m, k, ptr))

    def enable_edge_param_gradients(self):
        """Keep dLoss/d(edge parameters) from the next backward on (ign_batch_enable_edge_param_gradients;
        ``enable_training(edge_param_gradients=True)`` calls it).  A batch without it runs the default
        training step, launch for launch."""
        check(lib.ign_batch_enable_edge_param_gradients(self.engine.handle, self.handle))

    def edge_param_source_gradients(self, mp: int, source: int, out):
        """ign_batch_edge_param_gradients of one (mp, source) into the CUDA tensor ``out``."""
        check(lib.ign_batch_edge_param_gradients(self.engine.handle, self.handle, int(mp), int(source),
                                                 C.c_void_p(out.data_ptr())))
        return out

    def edge_param_gradients(self, adj: str, out=None):
        """dLoss/d(``params_<adj>``) after a completed backward, ``[n_edges, param_dim]`` in the batch's
        edge order, for the loss whose ``dpred`` that backward was given: the sum, in plan order, of
        ign_batch_edge_param_gradients over the MP sources that read the adjacency's parameters (each
        already summed over its MP's iterations).  The batch must have been opted in before that
        backward began (``enable_training(edge_param_gradients=True)`` or
        ``enable_edge_param_gradients``); nothing is enabled from here.  With ``out`` a contiguous
        float32 CUDA tensor it is filled on the engine's stream (torch's current stream is made to
        follow the plan's for the adds) and returned; else a float32 ndarray."""
        import torch
        ne, P, sources = self._edge_sources(adj)
        dev = "cuda:%d" % self.engine.device
        if out is not None:
            if not _is_device_tensor(out):
                raise ValueError("edge_param_gradients: out must be a CUDA tensor")
            _device_rows(out, ne, P, "edge_param_gradients")
        total = out if out is not None else torch.empty((ne, P), dtype=torch.float32, device=dev)
        if out is not None:
            torch.cuda.synchronize(dev)   # whatever torch queued on out, before the engine's stream writes it
        self.edge_param_source_gradients(*sources[0], out=total)
        if len(sources) > 1:
            part = torch.empty((ne, P), dtype=torch.float32, device=dev)
            for m, k in sources[1:]:
                self.edge_param_source_gradients(m, k, out=part)
                self.engine.synchronize()   # the adds run on torch's stream
                total.view(ne, P).add_(part)
                torch.cuda.synchronize(dev)
        if out is not None:
            return out
        self.engine.synchronize()
        return total.cpu().numpy()

    # ---- training -------------------------------------------------------------------------
    def enable_training(self, edge_param_gradients: bool = False):
        check(lib.ign_batch_enable_training(self.engine.handle, self.handle))
        if edge_param_gradients:
            self.enable_edge_param_gradients()

    def set_dropout(self, seed: int, step: int):
        """The Dropout mask stream of the next ``forward_train`` (ign_batch_set_dropout); never
        called: (0, 0)."""
        check(lib.ign_batch_set_dropout(self.handle, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF))

    def forward_train(self, to_host: bool = True):
        out = np.empty((self.predictions, self.output_units), np.float32) if to_host else None
        check(lib.ign_forward_train(self.engine.handle, self.handle,
                                    out.ctypes.data_as(C.c_void_p) if to_host else None))
        return out

    # stepped training step (edge-cut partitions: partition.EdgeCutTraining exchanges between steps)
    def forward_train_begin(self):
        check(lib.ign_forward_train_begin(self.engine.handle, self.handle))

    def forward_train_mp(self):
        check(lib.ign_forward_train_mp(self.engine.handle, self.handle))

    def forward_train_end(self, to_host: bool = True):
        out = np.empty((self.predictions, self.output_units), np.float32) if to_host else None
        check(lib.ign_forward_train_end(self.engine.handle, self.handle,
                                        out.ctypes.data_as(C.c_void_p) if to_host else None))
        return out

    def backward_begin(self, dpred, grads, l2_scale: float = 1.0):
        check(lib.ign_backward_begin(self.engine.handle, self.handle, _ptr(dpred), _ptr(grads), float(l2_scale)))

    def backward_mp(self):
        check(lib.ign_backward_mp(self.engine.handle, self.handle))

    def backward_end(self):
        check(lib.ign_backward_end(self.engine.handle, self.handle))

    def train_buffers(self, entity: str):
        """(state, gradient) device pointers of the entity's current version, [rows + halo][H]."""
        st, gr = C.c_void_p(), C.c_void_p()
        check(lib.ign_batch_train_buffers(self.handle, self.engine.plan.entities.index(entity), C.byref(st),
                                          C.byref(gr)))
        return st.value, gr.value

    def predictions_ptr(self) -> int:
        p = C.c_void_p()
        check(lib.ign_batch_predictions(self.handle, C.byref(p)))
        return p.value

    def backward(self, dpred, grads):
        """dpred, grads: device tensors ([predictions * units], [n_params])."""
        check(lib.ign_backward(self.engine.handle, self.handle, _ptr(dpred), _ptr(grads)))

    def resident_info(self) -> dict:
        """The graph-resident forward of this batch (decided when the batch is built; at its first
        forward under IGN_RESIDENT_EAGER=0): whether it runs, its form and LDS, and the per-launch
        cost model (ign_batch_resident_info)."""
        r = _lib.ResidentInfo()
        if not hasattr(lib, "ign_batch_resident_info"):   # an A/B build of an older tree (IGN_AB_LIB=1)
            return {"active": 0}
        check(lib.ign_batch_resident_info(self.handle, C.byref(r)))
        return {name: getattr(r, name) for name, _ in _lib.ResidentInfo._fields_}

    def state_slot(self, entity: str) -> int:
        s = C.c_int32()
        check(lib.ign_batch_state_slot(self.handle, self.engine.plan.entities.index(entity), C.byref(s)))
        return s.value

    def forward(self, to_host: bool = True):
        eng = self.engine
        if to_host:
            out = np.empty((self.predictions, self.output_units), np.float32)
            check(lib.ign_forward(eng.handle, self.handle, out.ctypes.data_as(C.c_void_p)))
            return out
        check(lib.ign_forward(eng.handle, self.handle, None))
        return None

    def state(self, entity: str) -> np.ndarray:
        p = self.engine.plan
        e = p.entities.index(entity)
        out = np.empty((self.rows[e], p.hidden[e]), np.float32)
        check(lib.ign_batch_state(self.engine.handle, self.handle, e, out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        h = getattr(self, "handle", None)
        if h:
            lib.ign_batch_destroy(h)
            self.handle = None
            eng = self.engine
            eng._open_batches -= 1
            if eng._open_batches == 0 and getattr(eng, "_close_pending", False):
                eng.close()

    def __del__(self):
        self.close()


def split_cuts(n_graphs: int, parts: int) -> list:
    """Boundaries of ``parts`` sub-batches of consecutive graphs (at most one per graph, at least
    one): sub-batch i is graphs [cuts[i], cuts[i + 1]), sizes differing by at most one."""
    if n_graphs < 1:
        raise ValueError("SplitBatch: no graphs")
    parts = max(1, min(int(parts), n_graphs))
    return [n_graphs * i // parts for i in range(parts + 1)]


class SplitBatch:
    """The graphs as ``parts`` sub-batches of consecutive graphs, sub-batch i on the engine's
    replica i (its own plan and HIP stream; replica 0 is the engine itself).  ``forward`` enqueues
    every sub-batch before waiting, so the kernels of different sub-batches co-run: the
    memory-bound sum update of one beside the issue-bound ordered update of another (DESIGN §3b'').
    The predictions are the batch's, in graph order, bitwise those of one ``Batch`` (graphs are
    independent: GM:712-724)."""

    def __init__(self, engine: Engine, graphs, parts: int = 2):
        graphs = list(graphs)
        cuts = split_cuts(len(graphs), parts)
        parts = len(cuts) - 1
        self.engine = engine
        self.engines = [engine] + engine.replicas(parts - 1)
        self.parts = [Batch(e, graphs[cuts[i]:cuts[i + 1]]) for i, e in enumerate(self.engines)]
        self.num_graphs = sum(b.num_graphs for b in self.parts)
        self.predictions = sum(b.predictions for b in self.parts)
        self.output_units = self.parts[0].output_units
        self.edges_per_forward = sum(b.edges_per_forward for b in self.parts)
        self.gru_steps_per_forward = sum(b.gru_steps_per_forward for b in self.parts)
        self.graph_predictions = np.concatenate([b.graph_predictions for b in self.parts])

    def forward(self, to_host: bool = True):
        self.engine.replicas(len(self.parts) - 1)   # re-sync replica parameters if they changed
        for b in self.parts:
            b.forward(to_host=False)
        if not to_host:
            return None
        out = np.empty((self.predictions, self.output_units), np.float32)
        row = 0
        for b in self.parts:
            check(lib.ign_batch_read_predictions(b.engine.handle, b.handle,
                                                 out[row:row + b.predictions].ctypes.data_as(C.c_void_p)))
            row += b.predictions
        return out

    def set_features(self, entity: str, values):
        """``Batch.set_features`` on every sub-batch with its graphs' rows of ``values`` (the rows of the
        whole batch, in graph order; a dict, an array or a CUDA tensor as there).  Inference only."""
        p = self.engine.plan
        if entity not in p.entities:
            raise ValueError("no entity %r (the model has %s)" % (entity, p.entities))
        e = p.entities.index(entity)
        rows = sum(b.rows[e] for b in self.parts)
        F = sum(size for _, size in p.features[e])
        if _is_device_tensor(values):
            whole = _device_rows(values, rows, F, "set_features").reshape(rows, F)
        else:
            whole = feature_rows(p.features[e], rows, values)
        row = 0
        for b in self.parts:
            b.set_features(entity, whole[row:row + b.rows[e]])
            row += b.rows[e]

    def set_edge_params(self, adj: str, values):
        """``Batch.set_edge_params`` on every sub-batch with its graphs' edges of ``values`` (the edges of
        the whole batch, in graph order; an array or a CUDA tensor as there)."""
        P, found = edge_param_sources(self.engine.plan, adj)
        counts = [int(b.graph_edges[:, found[0][2]].sum()) for b in self.parts]
        if _is_device_tensor(values):
            whole = _device_rows(values, sum(counts), P, "set_edge_params").reshape(sum(counts), P)
        else:
            whole = edge_param_rows(sum(counts), P, values)
        row = 0
        for b, n in zip(self.parts, counts):
            b.set_edge_params(adj, whole[row:row + n])
            row += n

    def edge_param_gradients(self, adj: str):
        """``Batch.edge_param_gradients`` of every sub-batch, concatenated in graph order: for a caller
        that runs training steps on ``parts`` itself (each opted in, each after its own backward)."""
        return np.concatenate([b.edge_param_gradients(adj) for b in self.parts], 0)

    def synchronize(self):
        for e in self.engines:
            e.synchronize()

    def close(self):
        for b in self.parts:
            b.close()

    def __del__(self):
        self.close()


def dropout_keep(seed: int, site: int, step: int, rows: int, units: int, rate: float) -> np.ndarray:
    """The keep mask [rows, units] (uint8) of Dropout site ``site`` on the host (ign_dropout_keep; no
    GPU): the mask the training forward applies under ``Batch.set_dropout(s, step)`` when ``seed`` is
    ``s`` xor the layer's own seed."""
    out = np.empty((rows, units), np.uint8)
    check(lib.ign_dropout_keep(int(seed) & 0xFFFFFFFFFFFFFFFF, int(site), int(step) & 0xFFFFFFFF, rows, units, rate,
                               out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def device_count() -> int:
    n = C.c_int32()
    lib.ign_device_count(C.byref(n))
    return n.value
