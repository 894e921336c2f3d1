// plan_json.cpp — ign_plan_create_json: model_description.json + dimensions -> plan, in C++.
//
// The same lowering as ignnition_amd/engine.py MPPlan.from_model_info over the model
// information that ignnition_amd/json_operations.py builds, so a caller without Python (a C, Go
// or Java binding) can create a plan from the files the reference reads:
//   JO:162-180   dimensions injected: feature sizes, extra_parameters = dims[adj_vector]
//   JO:184-245   semantic validation (unknown source / destination entity, nn_name, message input),
//                incl. the JO:214 quirk: only predict ops' nn_name are checked in the readout
//   JO:270-300   nn_name resolved: message / readout networks take nn_architecture, a recurrent
//                update takes the network's other keys
//   JO:326-350   readout list: only the five known op types are kept (their index is the
//                readout_model_<i> counter, GM:605-655)
//   AUX:641-698  sources (message list, default direct_assignation), AUX:869-1003 Dense layers
//                (default name layer_<i>_<type>_<role>, "None" activation = linear)
//   GM:235-382   one GRU cell per destination entity name, adjacency / interleave slots in
//                first-use order, one convolution / attention weight set per model (GM:288-300)
// The JSON schema itself (jsonschema in the reference) is not re-validated: structural errors
// surface as IGN_ERR_INVALID from the lowering.  ign_plan_describe_json returns what a caller
// needs to build batches and load parameters: entity / feature order, the input keys of every
// adjacency and interleave slot, and the parameter names in tensor order (engine.py
// MPPlan.param_specs).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "json.h"

using ign::json::JVal;

namespace {

struct LowerError {
  int code;
  std::string msg;
};
[[noreturn]] void invalid(const std::string& m) { throw LowerError{IGN_ERR_INVALID, m}; }
[[noreturn]] void unsupported(const std::string& m) { throw LowerError{IGN_ERR_UNSUPPORTED, m}; }

const JVal& need(const JVal& o, const char* key, const std::string& where) {
  const JVal* v = o.t == JVal::Obj ? o.get(key) : nullptr;
  if (!v) invalid(where + ": missing key '" + key + "'");
  return *v;
}
const JVal* opt(const JVal& o, const char* key) { return o.t == JVal::Obj ? o.get(key) : nullptr; }
std::string str(const JVal& v, const std::string& where) {
  if (v.t != JVal::Str) invalid(where + ": expected a string");
  return v.str;
}
const std::vector<JVal>& arr(const JVal& v, const std::string& where) {
  if (v.t != JVal::Arr) invalid(where + ": expected a list");
  return v.arr;
}
// Python int() / float() of a JSON number or numeric string
double number(const JVal& v, const std::string& where) {
  if (v.t == JVal::Num || v.t == JVal::Bool) return v.num;
  if (v.t == JVal::Str) {
    char* e = nullptr;
    const double d = strtod(v.str.c_str(), &e);
    if (e && e != v.str.c_str() && *e == 0) return d;
  }
  invalid(where + ": expected a number");
}
bool truthy(const JVal& v) {   // Python bool()
  switch (v.t) {
    case JVal::Null: return false;
    case JVal::Bool: case JVal::Num: return v.num != 0;
    case JVal::Str: return !v.str.empty();
    case JVal::Arr: return !v.arr.empty();
    default: return !v.obj.empty();
  }
}
std::string quote(const std::string& s) {
  std::string o = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') { o += '\\'; o += c; }
    else if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
    else o += c;
  }
  return o + "\"";
}

// _lib.ACT; at: the position (plan_lower.h's ACT_AT_*), which refuses what act_ok refuses there, by name
int activation(const JVal* a, const std::string& where, int at) {
  if (!a || a->t == JVal::Null) return IGN_ACT_LINEAR;
  const std::string s = str(*a, where);
  static const std::map<std::string, int> NEW = {{"elu", IGN_ACT_ELU}, {"softplus", IGN_ACT_SOFTPLUS},
                                                 {"softsign", IGN_ACT_SOFTSIGN}, {"exponential", IGN_ACT_EXPONENTIAL},
                                                 {"hard_sigmoid", IGN_ACT_HARD_SIGMOID}};
  if (NEW.count(s) && !act_ok(NEW.at(s), at)) unsupported("activation '" + s + "' not supported");
  if (s == "None" || s == "linear") return IGN_ACT_LINEAR;
  if (s == "relu") return IGN_ACT_RELU;
  if (s == "selu") return IGN_ACT_SELU;
  if (s == "sigmoid") return IGN_ACT_SIGMOID;
  if (s == "tanh") return IGN_ACT_TANH;
  if (NEW.count(s)) return NEW.at(s);
  unsupported("activation '" + s + "' not supported");
}

struct Layer {
  std::string name;
  ign_dense_desc d;
};

// A Dropout (rate > 0) or LayerNormalization layer of a readout stack (engine.py MPPlan's `extra`
// records); a stack's list holds them in the architecture's order
struct Extra {
  bool norm;
  int before;                  // the Dense layer it precedes; the stack's layer count = after the last one
  double rate = 0.0;           // Dropout
  uint64_t seed = 0;
  double epsilon = 1e-3;       // LayerNormalization
  bool center = true, scale = true;
  std::string name;
};

// Feed_forward_model (AUX:869-1003) + MPPlan._dense_layers.  extra: where the stack's Dropout and
// LayerNormalization layers go (a readout stack); null for a message-creation network, which takes
// none.  The default-name counter counts every layer, Dropout included.
std::vector<Layer> dense_layers(const JVal& architecture, const std::string& role, const char* what,
                                std::vector<Extra>* extra, int at) {
  std::vector<Layer> out;
  int counter = 0;
  for (const JVal& l : arr(architecture, std::string(what) + " nn_architecture")) {
    const std::string type = str(need(l, "type_layer", what), std::string(what) + " type_layer");
    if (type == "Dropout") {
      if (!extra)
        unsupported("message layer type Dropout is not lowered: a message-creation network would need a fresh mask "
                    "per iteration (Dropout is lowered in the readout's Dense stacks only)");
      for (auto& kv : l.obj)
        if (kv.first != "type_layer" && kv.first != "rate" && kv.first != "name" && kv.first != "seed")
          unsupported(std::string("Dropout option '") + kv.first + "' is not lowered");
      const double rate = number(need(l, "rate", "Dropout"), "Dropout rate");
      if (!(rate >= 0.0 && rate < 1.0)) invalid("Dropout rate must be in [0, 1), got " + std::to_string(rate));
      const JVal* sd = opt(l, "seed");
      const uint64_t seed = sd && sd->t != JVal::Null ? (uint64_t)(int64_t)number(*sd, "Dropout seed") : 0;
      if (rate > 0.0) {   // rate 0: no layer (TF returns x)
        extra->push_back({false, (int)out.size()});
        extra->back().rate = rate;
        extra->back().seed = seed;
      }
      ++counter;
      continue;
    }
    if (type == "LayerNormalization" && extra) {
      Extra n{true, (int)out.size()};
      for (auto& kv : l.obj) {
        const std::string& k = kv.first;
        if (k == "type_layer") continue;
        if (k == "name") n.name = str(kv.second, "layer name");
        else if (k == "epsilon") n.epsilon = number(kv.second, "LayerNormalization epsilon");
        else if (k == "center") n.center = truthy(kv.second);
        else if (k == "scale") n.scale = truthy(kv.second);
        else if (k == "axis" && kv.second.t == JVal::Num && kv.second.num == std::floor(kv.second.num)) {
          if (kv.second.num != -1 && kv.second.num != 1)   // the stacks' tensors are [rows, units]
            unsupported("LayerNormalization axis " + std::to_string((long long)kv.second.num) +
                        " is not lowered (the last axis only: -1 or 1)");
        } else {
          unsupported("LayerNormalization option '" + k + "' is not lowered");
        }
      }
      if (!(n.epsilon >= 0.0)) invalid("LayerNormalization epsilon must be >= 0, got " + std::to_string(n.epsilon));
      if (n.name.empty()) n.name = "layer_" + std::to_string(counter) + "_" + type + "_" + role;
      extra->push_back(n);
      ++counter;
      continue;
    }
    if (type != "Dense")
      unsupported(std::string(what) + " layer type " + type + " is not lowered (" +
                  (extra ? "Dense, Dropout and LayerNormalization" : "Dense") + " only)");
    for (auto& kv : l.obj)
      if (kv.first != "type_layer" && kv.first != "units" && kv.first != "activation" &&
          kv.first != "kernel_regularizer" && kv.first != "name" && kv.first != "use_bias")
        unsupported(std::string("Dense option '") + kv.first + "' is not lowered");
    Layer y;
    const JVal* nm = opt(l, "name");
    y.name = nm ? str(*nm, "layer name") : "layer_" + std::to_string(counter) + "_" + type + "_" + role;
    y.d.units = (int32_t)number(need(l, "units", what), "units");
    y.d.activation = activation(opt(l, "activation"), "activation", at);
    const JVal* ub = opt(l, "use_bias");
    y.d.use_bias = ub ? (truthy(*ub) ? 1 : 0) : 1;
    const JVal* kr = opt(l, "kernel_regularizer");
    y.d.l2 = kr && truthy(*kr) ? (float)number(*kr, "kernel_regularizer") : 0.f;
    out.push_back(y);
    ++counter;
  }
  for (bool norm : {false, true})
    for (size_t i = 0; extra && out.empty() && i < extra->size(); ++i)
      if ((*extra)[i].norm == norm)
        invalid(std::string(what) + " network has a " + (norm ? "LayerNormalization" : "Dropout") + " but no Dense layer");
  return out;
}

struct Net {             // message-creation network of one source (engine.py _message_net)
  std::vector<int32_t> inputs;
  int param_dim = 0, din = 0;
  std::string prefix;
  std::vector<Layer> layers;
};

struct AdjSlot {
  std::string adj, src, dst;
  bool operator==(const AdjSlot& o) const { return adj == o.adj && src == o.src && dst == o.dst; }
};

struct Lowered {
  int T = 0;
  std::vector<std::string> ents;
  std::vector<int> hidden;
  std::vector<std::vector<std::pair<std::string, int>>> features;
  std::vector<AdjSlot> adj;
  std::vector<std::string> il;
  struct Src {
    int entity, adjacency, interleave;
    bool has_net;
    Net net;
  };
  struct MP {
    int dst, aggr, axis, cell, act;
    std::vector<Src> srcs;
  };
  std::vector<MP> mps;
  std::vector<std::pair<std::string, std::pair<int, int>>> cells;   // dst name, (din, H)
  std::vector<ign_cell_options> cell_opts;                          // per cell (ign_plan_set_cell_options)
  int conv_dim = 0, attn_dim = 0;
  struct RoOp {
    int type, mode = 0, adj = -1, counter = 0, in_width = 0;
    std::vector<int32_t> inputs;
    std::vector<Layer> layers;
    std::vector<Extra> extra;
  };
  std::vector<RoOp> ro_ops;
  std::vector<int32_t> ro_inputs;
  std::vector<int> ro_widths;
  int predict_counter = 0;
  std::string label;
  std::vector<Layer> dense;
  std::vector<Extra> extra;   // the predict network's

  std::vector<std::pair<std::string, std::vector<int64_t>>> param_specs() const {
    std::vector<std::pair<std::string, std::vector<int64_t>>> s;
    for (size_t k = 0; k < cells.size(); ++k) {
      const auto& c = cells[k];
      const int din = c.second.first, h = c.second.second;
      s.push_back({c.first + "_update/kernel", {din, 3 * h}});
      s.push_back({c.first + "_update/recurrent_kernel", {h, 3 * h}});
      // Keras' GRUCell: [2][3H]; reset_after false, [3H]; use_bias false, no variable
      if (cell_opts[k].use_bias && cell_opts[k].reset_after) s.push_back({c.first + "_update/bias", {2, 3 * h}});
      else if (cell_opts[k].use_bias) s.push_back({c.first + "_update/bias", {3 * h}});
    }
    for (auto& m : mps)
      for (auto& sr : m.srcs) {
        if (!sr.has_net) continue;
        int fan = sr.net.din;
        for (auto& l : sr.net.layers) {
          s.push_back({sr.net.prefix + l.name + "/kernel", {fan, l.d.units}});
          if (l.d.use_bias) s.push_back({sr.net.prefix + l.name + "/bias", {l.d.units}});
          fan = l.d.units;
        }
      }
    if (conv_dim) s.push_back({"convolution/kernel", {conv_dim, conv_dim}});
    if (attn_dim) {
      s.push_back({"attention/kernel1", {attn_dim, attn_dim}});
      s.push_back({"attention/kernel2", {attn_dim, attn_dim}});
      s.push_back({"attention/attn_kernel", {2 * attn_dim, 1}});
    }
    // a stack's tensors: each LayerNormalization's gamma / beta in front of the Dense layer it precedes
    auto stack = [&](int counter, int fan, const std::vector<Layer>& layers, const std::vector<Extra>& extra) {
      const std::string model = "readout_model_" + std::to_string(counter) + "/";
      for (size_t li = 0; li <= layers.size(); ++li) {
        for (const Extra& n : extra) {   // (in the architecture's order)
          if (!n.norm || n.before != (int)li) continue;
          if (n.scale) s.push_back({model + n.name + "/gamma", {fan}});
          if (n.center) s.push_back({model + n.name + "/beta", {fan}});
        }
        if (li == layers.size()) break;
        const auto& l = layers[li];
        s.push_back({model + l.name + "/kernel", {fan, l.d.units}});
        if (l.d.use_bias) s.push_back({model + l.name + "/bias", {l.d.units}});
        fan = l.d.units;
      }
    };
    for (auto& op : ro_ops) stack(op.counter, op.in_width, op.layers, op.extra);
    int fan = 0;
    for (int i : ro_inputs) fan += ro_widths[i];
    stack(predict_counter, fan, dense, extra);
    return s;
  }
};

// JO:184-245
void validate(const JVal& data) {
  std::vector<std::string> src_names, dst_names, called, input_names;
  std::vector<std::string> output_names = {"hs_source", "hs_dest", "edge_params"};
  for (const JVal& stage : arr(need(need(data, "message_passing", "model"), "stages", "message_passing"), "stages"))
    for (const JVal& mp : arr(need(stage, "stage_mp", "stage"), "stage_mp")) {
      dst_names.push_back(str(need(mp, "destination_entity", "message passing"), "destination_entity"));
      for (const JVal& src : arr(need(mp, "source_entities", "message passing"), "source_entities")) {
        src_names.push_back(str(need(src, "name", "source entity"), "source name"));
        if (const JVal* msg = opt(src, "message"))
          for (const JVal& op : arr(*msg, "message")) {
            if (str(need(op, "type", "message operation"), "type") == "neural_network") {
              called.push_back(str(need(op, "nn_name", "message operation"), "nn_name"));
              if (const JVal* in = opt(op, "input"))
                for (const JVal& i : arr(*in, "input")) input_names.push_back(str(i, "input"));
            }
            if (const JVal* o = opt(op, "output_name")) output_names.push_back(str(*o, "output_name"));
          }
      }
    }
  for (const JVal& op : arr(need(data, "readout", "model"), "readout"))
    if (str(need(op, "type", "readout operation"), "type") == "predict")
      called.push_back(str(need(op, "nn_name", "predict"), "nn_name"));
  std::vector<std::string> entity_names, nn_names;
  for (const JVal& e : arr(need(data, "entities", "model"), "entities")) entity_names.push_back(str(need(e, "name", "entity"), "name"));
  for (const JVal& n : arr(need(data, "neural_networks", "model"), "neural_networks"))
    nn_names.push_back(str(need(n, "nn_name", "neural network"), "nn_name"));
  auto has = [](const std::vector<std::string>& v, const std::string& x) {
    for (auto& y : v) if (y == x) return true;
    return false;
  };
  for (auto& a : src_names)
    if (!has(entity_names, a))
      invalid("IGNNITION: The source entity " + a + " was used in a message passing. However, there is no such "
              "entity. \n Please check the spelling or define a new entity.");
  for (auto& d : dst_names)
    if (!has(entity_names, d))
      invalid("IGNNITION: The destination entity " + d + " was used in a message passing. However, there is no "
              "such entity. \n Please check the spelling or define a new entity.");
  for (auto& n : called)
    if (!has(nn_names, n))
      invalid("IGNNITION: The name " + n + " is used as a reference to a neural network (nn_name), even though the "
              "neural network was not defined. \n Please make sure the name is correctly spelled or define a neural "
              "network named " + n);
  for (auto& i : input_names)
    if (!has(output_names, i))
      invalid("IGNNITION: The name " + i + " was used as input of a message creation operation even though it "
              "wasn't the output of one.");
}

Lowered lower(const JVal& data, const JVal& dims) {
  validate(data);
  auto dim = [&](const std::string& key) -> int {
    const JVal* v = opt(dims, key.c_str());
    if (!v) invalid("dimensions: no entry for '" + key + "' (JO:162-180)");
    return (int)number(*v, "dimension of " + key);
  };
  std::map<std::string, const JVal*> nets;
  for (const JVal& n : arr(need(data, "neural_networks", "model"), "neural_networks"))
    nets[str(need(n, "nn_name", "neural network"), "nn_name")] = &n;   // JO _get_nn_mapping: last wins
  Lowered p;
  p.T = (int)number(need(need(data, "message_passing", "model"), "num_iterations", "message_passing"), "num_iterations");
  std::map<std::string, int> eidx;
  for (const JVal& e : arr(need(data, "entities", "model"), "entities")) {
    const std::string name = str(need(e, "name", "entity"), "name");
    const double h = number(need(e, "hidden_state_dimension", "entity " + name), "hidden_state_dimension");
    if (h != std::floor(h)) unsupported("non-integer hidden_state_dimension");
    eidx[name] = (int)p.ents.size();
    p.ents.push_back(name);
    p.hidden.push_back((int)h);
    std::vector<std::pair<std::string, int>> fs;
    if (const JVal* f = opt(e, "features"))
      for (const JVal& x : arr(*f, "features")) {
        const std::string fn = str(need(x, "name", "feature"), "feature name");
        fs.push_back({fn, dim(fn)});
      }
    p.features.push_back(fs);
  }
  std::map<std::string, int> cell_of;
  for (const JVal& stage : arr(need(need(data, "message_passing", "model"), "stages", "message_passing"), "stages"))
    for (const JVal& mp : arr(need(stage, "stage_mp", "stage"), "stage_mp")) {
      const std::string dst = mp.get("destination_entity")->str;
      const JVal& upd = need(mp, "update", "message passing");
      const std::string ut = str(need(upd, "type", "update"), "update type");
      if (ut != "recurrent_neural_network")
        unsupported("feed-forward update is not executable in the reference (GM:338)");
      const std::string un = str(need(upd, "nn_name", "update"), "nn_name");
      const JVal* arch = nets.count(un) ? nets[un] : nullptr;
      if (!arch) invalid("update nn_name '" + un + "' is not defined");
      // JO:287-291: the network's keys other than nn_name / nn_type join the update dict
      // of GRUCell's keys the four of ign_plan_set_cell_options are lowered (absent: the Keras default)
      std::string rtype;
      std::vector<std::string> extra;
      ign_cell_options copt{IGN_ACT_TANH, IGN_ACT_SIGMOID, 1, 1};
      const JVal *act_v = nullptr, *ract_v = nullptr;   // (named after the refusal of other keys, as engine.py)
      auto cell_key = [&](const std::string& k, const JVal& v) {
        if (k == "units" || k == "name") return;
        if (k == "activation") act_v = &v;
        else if (k == "recurrent_activation") ract_v = &v;
        else if (k == "use_bias") copt.use_bias = truthy(v);
        else if (k == "reset_after") copt.reset_after = truthy(v);
        else extra.push_back(k);
      };
      for (auto& kv : arch->obj) {
        if (kv.first == "nn_name" || kv.first == "nn_type") continue;
        if (kv.first == "recurrent_type") rtype = str(kv.second, "recurrent_type");
      }
      if (rtype == "GRU") {   // (any other type is refused below, before its keys are read)
        for (auto& kv : arch->obj)
          if (kv.first != "nn_name" && kv.first != "nn_type" && kv.first != "recurrent_type") cell_key(kv.first, kv.second);
        for (auto& kv : upd.obj)
          if (kv.first != "type" && kv.first != "nn_name" && kv.first != "recurrent_type") cell_key(kv.first, kv.second);
      }
      if (rtype != "GRU")
        unsupported("recurrent_type " + rtype + " is not lowered (only GRU; LSTM passes one state, AUX:764)");
      if (!extra.empty()) {
        std::sort(extra.begin(), extra.end());
        std::string e = "GRU options [";
        for (size_t i = 0; i < extra.size(); ++i) e += (i ? ", '" : "'") + extra[i] + "'";
        unsupported(e + "] are not lowered (Keras defaults only)");
      }
      if (act_v) copt.activation = activation(act_v, "GRU activation", ACT_AT_PREDICT);
      if (ract_v) copt.recurrent_activation = activation(ract_v, "GRU recurrent_activation", ACT_AT_PREDICT);
      const JVal& ag = need(mp, "aggregation", "message passing");
      const std::string aggr = str(need(ag, "type", "aggregation"), "aggregation type");
      static const std::map<std::string, int> AGG = {{"sum", IGN_AGGR_SUM}, {"ordered", IGN_AGGR_ORDERED},
                                                     {"interleave", IGN_AGGR_INTERLEAVE}, {"concat", IGN_AGGR_CONCAT},
                                                     {"attention", IGN_AGGR_ATTENTION},
                                                     {"convolution", IGN_AGGR_CONVOLUTION}};
      if (!AGG.count(aggr)) unsupported("aggregation '" + aggr + "' is not lowered yet");
      int act = 0;
      if (aggr == "convolution") {   // AUX:370-374: activation_function, default relu
        const JVal* f = opt(ag, "activation_function");
        const std::string fn = f ? str(*f, "activation_function") : "relu";
        JVal tmp;
        tmp.t = JVal::Str;
        tmp.str = fn;
        act = activation(&tmp, "convolution activation", ACT_AT_CONVOLUTION);
      }
      const int axis = aggr == "concat" ? (int)number(need(ag, "concat_axis", "concat"), "concat_axis") : 0;
      const bool feature_concat = aggr == "concat" && axis == 2;
      Lowered::MP m;
      m.dst = eidx.at(dst);
      m.aggr = AGG.at(aggr);
      m.axis = axis;
      m.act = act;
      int din = -1;
      for (const JVal& s : arr(need(mp, "source_entities", "message passing"), "source_entities")) {
        Lowered::Src sr;
        const std::string sname = s.get("name")->str;
        const std::string adjv = str(need(s, "adj_vector", "source " + sname), "adj_vector");
        const int extra_params = dim(adjv);
        sr.entity = eidx.at(sname);
        sr.has_net = false;
        // message formation (AUX:641-698; engine.py _message_net)
        std::vector<const JVal*> nn_ops;
        int op_counter = 0, net_counter = -1;
        if (const JVal* msg = opt(s, "message"))
          for (const JVal& op : arr(*msg, "message")) {
            if (op.get("type")->str == "neural_network") {
              nn_ops.push_back(&op);
              net_counter = op_counter;
            }
            ++op_counter;
          }
        if (nn_ops.size() > 1)
          unsupported("more than one message network per source (the reference cannot chain them, GM:458/470)");
        if (!nn_ops.empty()) {
          const JVal& op = *nn_ops[0];
          sr.has_net = true;
          Net& net = sr.net;
          const std::map<std::string, int> WIDTH = {{"hs_source", p.hidden[sr.entity]}, {"hs_dest", p.hidden[m.dst]},
                                                    {"edge_params", extra_params}};
          if (const JVal* in = opt(op, "input"))
            for (const JVal& i : arr(*in, "input")) {
              const std::string x = str(i, "message input");
              if (!WIDTH.count(x)) unsupported("message input '" + x + "' is not readable in the reference (GM:458/470)");
              net.inputs.push_back(x == "hs_source" ? IGN_MSG_HS_SOURCE : x == "hs_dest" ? IGN_MSG_HS_DEST
                                                                                          : IGN_MSG_EDGE_PARAMS);
              net.din += WIDTH.at(x);
            }
          const JVal* arch_n = nets[str(need(op, "nn_name", "message network"), "nn_name")];
          net.layers = dense_layers(need(*arch_n, "nn_architecture", "message network"),
                                    "message_creation_" + std::to_string(net_counter), "message", nullptr, ACT_AT_MESSAGE);
          net.param_dim = extra_params;
          net.prefix = sname + "_to_" + dst + "_message_creation_0/";
        }
        AdjSlot slot{adjv, sname, dst};
        int a = -1;
        for (size_t k = 0; k < p.adj.size(); ++k)
          if (p.adj[k] == slot) a = (int)k;
        if (a < 0) { a = (int)p.adj.size(); p.adj.push_back(slot); }
        sr.adjacency = a;
        sr.interleave = -1;
        if (aggr == "interleave") {
          const std::string key = "indices_" + sname + "_to_" + dst;
          int il = -1;
          for (size_t k = 0; k < p.il.size(); ++k)
            if (p.il[k] == key) il = (int)k;
          if (il < 0) { il = (int)p.il.size(); p.il.push_back(key); }
          sr.interleave = il;
        }
        const int msg_dim = sr.has_net ? sr.net.layers.back().d.units : p.hidden[sr.entity];
        din = feature_concat ? (din < 0 ? 0 : din) + msg_dim : msg_dim;   // axis-2 concat (AUX:443-456)
        m.srcs.push_back(sr);
      }
      if (!cell_of.count(dst)) {
        cell_of[dst] = (int)p.cells.size();
        p.cells.push_back({dst, {din, p.hidden[m.dst]}});
        p.cell_opts.push_back(copt);   // one cell per destination entity (GM:309-313): its first MP's keys
      }
      m.cell = cell_of[dst];
      if (aggr == "convolution") p.conv_dim = p.hidden[m.dst];   // GM:288-300: the last MP's weights
      if (aggr == "attention") p.attn_dim = p.hidden[m.dst];
      p.mps.push_back(m);
    }
  // readout (engine.py MPPlan._lower_readout): names resolve to entity states, then op outputs
  std::map<std::string, int> names = eidx;
  std::vector<std::string> spaces;   // "e<i>" / "graph" / "adj<k>"
  for (size_t i = 0; i < p.ents.size(); ++i) {
    p.ro_widths.push_back(p.hidden[i]);
    spaces.push_back("e" + std::to_string(i));
  }
  auto resolve = [&](const JVal& n) {
    const std::string s = str(n, "readout input");
    if (!names.count(s))
      unsupported("readout input '" + s + "' is not an entity state or a readout output (raw input features are "
                  "not lowered as readout inputs)");
    return names.at(s);
  };
  auto add = [&](const std::string& name, int width, const std::string& space) {
    names[name] = (int)p.ro_widths.size();
    p.ro_widths.push_back(width);
    spaces.push_back(space);
  };
  int counter = 0;
  const JVal* pred = nullptr;
  for (const JVal& op : arr(need(data, "readout", "model"), "readout")) {
    const std::string t = op.get("type")->str;
    if (t != "predict" && t != "pooling" && t != "product" && t != "neural_network" && t != "extend_adjacencies")
      continue;   // JO:326-350 keeps only these
    if (t == "predict") {
      pred = &op;
      p.predict_counter = counter;
      break;
    }
    Lowered::RoOp d;
    d.counter = counter;
    for (const JVal& i : arr(need(op, "input", "readout operation"), "input")) d.inputs.push_back(resolve(i));
    if (d.inputs.empty()) invalid("readout operation without inputs");
    const std::string first = spaces[d.inputs[0]];
    if (t == "neural_network") {
      d.type = IGN_RO_NEURAL_NETWORK;
      const std::string nn = str(need(op, "nn_name", "readout neural_network"), "nn_name");
      if (!nets.count(nn)) invalid("readout nn_name '" + nn + "' is not defined");
      d.layers = dense_layers(need(*nets[nn], "nn_architecture", "readout network"), "readout", "readout", &d.extra, ACT_AT_READOUT_OP);
      for (int i : d.inputs) d.in_width += p.ro_widths[i];
      const JVal* on = opt(op, "output_name");
      add(on ? str(*on, "output_name") : "None", d.layers.back().d.units, first);
    } else if (t == "pooling") {
      d.type = IGN_RO_POOLING;
      const std::string tp = str(need(op, "type_pooling", "pooling"), "type_pooling");
      if (tp == "sum") d.mode = IGN_POOL_SUM;
      else if (tp == "mean") d.mode = IGN_POOL_MEAN;
      else if (tp == "max") d.mode = IGN_POOL_MAX;
      else unsupported("pooling type '" + tp + "' is not lowered");
      add(str(need(op, "output_name", "pooling"), "output_name"), p.ro_widths[d.inputs[0]], "graph");
    } else if (t == "product") {
      d.type = IGN_RO_PRODUCT;
      const std::string tp = str(need(op, "type_product", "product"), "type_product");
      if (tp != "element_wise")
        unsupported("product '" + tp + "' is not lowered: tf.tensordot(axes=0) is a rank-4 outer product that the "
                    "reference records as width 1 (GM:374-375)");
      if (d.inputs.size() < 2) unsupported("product needs two inputs");
      const std::string space = first != "graph" ? first : spaces[d.inputs[1]];
      add(str(need(op, "output_name", "product"), "output_name"), p.ro_widths[d.inputs[0]], space);
    } else {
      d.type = IGN_RO_EXTEND;
      const std::string al = str(need(op, "adj_list", "extend_adjacencies"), "adj_list");
      for (size_t k = 0; k < p.adj.size() && d.adj < 0; ++k)
        if (p.adj[k].adj == al) d.adj = (int)k;
      if (d.adj < 0)
        unsupported("extend_adjacencies: adjacency '" + al + "' is not read by any message passing (the reference's "
                    "input has no src_/dst_ for it)");
      if (d.inputs.size() < 2) invalid("extend_adjacencies needs two inputs");
      const std::string sp = "adj" + std::to_string(d.adj);
      add(str(need(op, "output_name_src", "extend_adjacencies"), "output_name_src"), p.ro_widths[d.inputs[0]], sp);
      add(str(need(op, "output_name_dst", "extend_adjacencies"), "output_name_dst"), p.ro_widths[d.inputs[1]], sp);
    }
    p.ro_ops.push_back(d);
    ++counter;
  }
  if (!pred) unsupported("the readout has no predict operation");
  p.label = str(need(*pred, "label", "predict"), "label");
  for (const JVal& i : arr(need(*pred, "input", "predict"), "input")) p.ro_inputs.push_back(resolve(i));
  const std::string nn = pred->get("nn_name")->str;
  p.dense = dense_layers(need(*nets[nn], "nn_architecture", "predict network"), "readout", "readout", &p.extra, ACT_AT_PREDICT);
  return p;
}

// m: the plan lowered from p, its Dropout and LayerNormalization layers added
std::string describe(const Lowered& p, const PlanModel& m) {
  std::string s = "{\"iterations\": " + std::to_string(p.T) + ", \"entities\": [";
  for (size_t e = 0; e < p.ents.size(); ++e) {
    s += (e ? ", " : "") + std::string("{\"name\": ") + quote(p.ents[e]) + ", \"hidden\": " + std::to_string(p.hidden[e]) +
         ", \"features\": [";
    for (size_t f = 0; f < p.features[e].size(); ++f)
      s += (f ? ", [" : "[") + quote(p.features[e][f].first) + ", " + std::to_string(p.features[e][f].second) + "]";
    s += "]}";
  }
  s += "], \"adjacencies\": [";
  for (size_t k = 0; k < p.adj.size(); ++k)
    s += (k ? ", " : "") + std::string("{\"adj\": ") + quote(p.adj[k].adj) + ", \"src\": " + quote(p.adj[k].src) +
         ", \"dst\": " + quote(p.adj[k].dst) + ", \"keys\": [" + quote("src_" + p.adj[k].adj) + ", " +
         quote("dst_" + p.adj[k].adj) + ", " + quote("seq_" + p.adj[k].src + "_" + p.adj[k].dst) + "]}";
  s += "], \"interleave\": [";
  for (size_t k = 0; k < p.il.size(); ++k) s += (k ? ", " : "") + quote(p.il[k]);
  s += "], \"label\": " + quote(p.label) + ", \"params\": [";
  const auto specs = p.param_specs();
  for (size_t i = 0; i < specs.size(); ++i) {
    s += (i ? ", " : "") + std::string("{\"name\": ") + quote(specs[i].first) + ", \"shape\": [";
    for (size_t d = 0; d < specs[i].second.size(); ++d) s += (d ? ", " : "") + std::to_string(specs[i].second[d]);
    s += "]}";
  }
  // Dropout sites in site order (readout operations in order, then predict): stack = the
  // operation's index among the lowered operations (ign_plan_add_dropout's), -1 for predict
  s += "], \"dropout\": [";
  for (size_t i = 0; i < m.drops.size(); ++i) {
    const DropSite& x = m.drops[i];
    char rate[32];
    snprintf(rate, sizeof rate, "%.9g", (double)x.rate);
    s += (i ? ", " : "") + std::string("{\"site\": ") + std::to_string(i) + ", \"stack\": " + std::to_string(x.stack) +
         ", \"before_layer\": " + std::to_string(x.before) + ", \"rate\": " + rate + ", \"seed\": " +
         std::to_string(x.seed) + "}";
  }
  // LayerNormalization layers in the same order, numbered on their own; order = the layer's place
  // among the Dropout sites and LayerNormalization layers in front of the same Dense layer.  The
  // names, in site order: a stack's list already holds its layers by position
  std::vector<std::string> names;
  auto name = [&](const std::vector<Extra>& extra) {
    for (const Extra& e : extra)
      if (e.norm) names.push_back(e.name);
  };
  for (auto& op : p.ro_ops) name(op.extra);
  name(p.extra);
  s += "], \"layernorm\": [";
  for (size_t i = 0; i < m.norms.size(); ++i) {
    const NormSite& x = m.norms[i];
    char eps[32];
    snprintf(eps, sizeof eps, "%.9g", (double)x.epsilon);
    s += (i ? ", " : "") + std::string("{\"site\": ") + std::to_string(i) + ", \"stack\": " + std::to_string(x.stack) +
         ", \"before_layer\": " + std::to_string(x.before) + ", \"order\": " +
         std::to_string(site_order(&m, x.stack, SL_LAYERNORM, (int)i)) + ", \"epsilon\": " + eps + ", \"center\": " +
         (x.center ? "true" : "false") + ", \"scale\": " + (x.scale ? "true" : "false") + ", \"units\": " +
         std::to_string(x.units) + ", \"name\": " + quote(names[i]) + "}";
  }
  // The activation codes (ign_activation) the plan carries, by position: predict's Dense layers, each
  // readout operation's (empty unless a neural_network), each MP's message networks per source, and
  // each MP's convolution activation_function (0 for another aggregation)
  auto codes = [](const std::vector<DenseP>& layers) {
    std::string o = "[";
    for (size_t l = 0; l < layers.size(); ++l) o += (l ? ", " : "") + std::to_string(layers[l].act);
    return o + "]";
  };
  s += "], \"activations\": {\"predict\": " + codes(m.dense) + ", \"readout_ops\": [";
  for (size_t k = 0; k < m.ro_ops.size(); ++k) s += (k ? ", " : "") + codes(m.ro_ops[k].layers);
  s += "], \"message\": [";
  for (size_t i = 0; i < m.mps.size(); ++i) {
    s += i ? ", [" : "[";
    for (size_t q = 0; q < m.mps[i].nn.size(); ++q) s += (q ? ", " : "") + codes(m.mps[i].nn[q].layers);
    s += "]";
  }
  s += "], \"convolution\": [";
  for (size_t i = 0; i < m.mps.size(); ++i) s += (i ? ", " : "") + std::to_string(m.mps[i].act);
  // the GRU cells as the plan carries them (ign_plan_set_cell_options), in cell order
  s += "]}, \"cells\": [";
  for (size_t c = 0; c < m.cells.size(); ++c) {
    const CellP& cp = m.cells[c];
    s += (c ? ", " : "") + std::string("{\"name\": ") + quote(p.cells[c].first) + ", \"input_dim\": " +
         std::to_string(cp.din) + ", \"units\": " + std::to_string(cp.H) + ", \"activation\": " +
         std::to_string(cp.act) + ", \"recurrent_activation\": " + std::to_string(cp.ract) + ", \"use_bias\": " +
         (cp.use_bias ? "true" : "false") + ", \"reset_after\": " + (cp.reset_after ? "true" : "false") + "}";
  }
  return s + "]}";
}

}  // namespace

int ign_plan_create_json(const char* model_json, const char* dims_json, int32_t device, ign_plan** out) {
  if (!model_json || !dims_json || !out) return fail(IGN_ERR_INVALID, "null argument");
  *out = nullptr;
  Lowered p;
  try {
    const JVal data = ign::json::Parser(model_json, model_json + strlen(model_json), "model_description.json").parse();
    const JVal dims = ign::json::Parser(dims_json, dims_json + strlen(dims_json), "dimensions").parse();
    if (data.t != JVal::Obj) invalid("model_description.json is not an object");
    if (dims.t != JVal::Obj) invalid("dimensions are not an object");
    p = lower(data, dims);
  } catch (const ign::json::JsonError& e) {
    return fail(IGN_ERR_INVALID, "%s", e.what());
  } catch (const LowerError& e) {
    return fail(e.code, "%s", e.msg.c_str());
  } catch (const std::exception& e) {
    return fail(IGN_ERR_INVALID, "model description: %s", e.what());
  }
  // the C structures (engine.py MPPlan.to_desc)
  std::vector<ign_entity_desc> ents;
  for (size_t e = 0; e < p.ents.size(); ++e) {
    int ft = 0;
    for (auto& f : p.features[e]) ft += f.second;
    ents.push_back({p.hidden[e], ft});
  }
  std::vector<std::vector<ign_source_desc>> srcs(p.mps.size());
  std::vector<std::vector<ign_dense_desc>> msg_layers;
  msg_layers.reserve(64);
  std::vector<ign_mp_desc> mps;
  for (size_t i = 0; i < p.mps.size(); ++i) {
    const auto& m = p.mps[i];
    for (const auto& sr : m.srcs) {
      ign_source_desc sd{};
      sd.entity = sr.entity;
      sd.adjacency = sr.adjacency;
      sd.interleave = sr.interleave;
      if (sr.has_net) {
        msg_layers.emplace_back();
        for (auto& l : sr.net.layers) msg_layers.back().push_back(l.d);
        sd.msg_num_inputs = (int32_t)sr.net.inputs.size();
        sd.msg_inputs = sr.net.inputs.data();
        sd.msg_param_dim = sr.net.param_dim;
        sd.msg_num_layers = (int32_t)sr.net.layers.size();
        sd.msg_layers = msg_layers.back().data();
      }
      srcs[i].push_back(sd);
    }
    mps.push_back({m.dst, m.aggr, m.axis, m.cell, (int32_t)m.srcs.size(), srcs[i].data(), m.act});
  }
  std::vector<ign_cell_desc> cells;
  for (auto& c : p.cells) cells.push_back({c.second.first, c.second.second});
  std::vector<ign_dense_desc> dense;
  for (auto& l : p.dense) dense.push_back(l.d);
  std::vector<std::vector<ign_dense_desc>> ro_layers(p.ro_ops.size());
  std::vector<ign_readout_op_desc> rops;
  for (size_t k = 0; k < p.ro_ops.size(); ++k) {
    const auto& op = p.ro_ops[k];
    for (auto& l : op.layers) ro_layers[k].push_back(l.d);
    rops.push_back({op.type, (int32_t)op.inputs.size(), op.inputs.data(), op.mode, op.adj,
                    (int32_t)op.layers.size(), ro_layers[k].data()});
  }
  ign_plan_desc d{};
  d.num_iterations = p.T;
  d.num_entities = (int32_t)ents.size();
  d.entities = ents.data();
  d.num_adjacencies = (int32_t)p.adj.size();
  d.num_interleave = (int32_t)p.il.size();
  d.num_mps = (int32_t)mps.size();
  d.mps = mps.data();
  d.num_cells = (int32_t)cells.size();
  d.cells = cells.data();
  d.num_readout_inputs = (int32_t)p.ro_inputs.size();
  d.readout_inputs = p.ro_inputs.data();
  d.num_dense = (int32_t)dense.size();
  d.dense = dense.data();
  d.num_readout_ops = (int32_t)rops.size();
  d.readout_ops = rops.data();
  ign_plan* plan = nullptr;
  int rc = ign_plan_create(&d, device, &plan);
  if (rc) return rc;
  // the Dropout and LayerNormalization layers (ign_plan_add_dropout's and ign_plan_add_layernorm's
  // routines), each stack's in the architecture's order
  auto add_sites = [&](int stack, const std::vector<Extra>& extra) {
    for (size_t i = 0; !rc && i < extra.size(); ++i) {
      const Extra& e = extra[i];
      rc = e.norm ? plan_add_layernorm(plan, stack, e.before, (float)e.epsilon, e.center, e.scale)
                  : plan_add_dropout(plan, stack, e.before, (float)e.rate, e.seed);
    }
  };
  for (size_t k = 0; k < p.ro_ops.size(); ++k) add_sites((int)k, p.ro_ops[k].extra);
  add_sites(-1, p.extra);
  for (size_t c = 0; !rc && c < p.cell_opts.size(); ++c) rc = plan_set_cell_options(plan, (int)c, &p.cell_opts[c]);
  if (rc) {
    ign_plan_destroy(plan);
    return rc;
  }
  const auto specs = p.param_specs();
  int32_t nt = 0;
  ign_plan_num_param_tensors(plan, &nt);
  if ((size_t)nt != specs.size()) {
    ign_plan_destroy(plan);
    return fail(IGN_ERR_INVALID, "internal: %zu parameter names for %d tensors", specs.size(), nt);
  }
  plan->describe = describe(p, *plan);
  *out = plan;
  return IGN_OK;
}

int ign_plan_describe_json(const ign_plan* plan, char* buf, int64_t size, int64_t* needed) {
  if (!plan) return fail(IGN_ERR_INVALID, "null plan");
  if (plan->describe.empty()) return fail(IGN_ERR_INVALID, "only plans from ign_plan_create_json carry a description");
  const int64_t n = (int64_t)plan->describe.size() + 1;
  if (needed) *needed = n;
  if (buf && size > 0) {
    const int64_t k = std::min<int64_t>(n - 1, size - 1);
    memcpy(buf, plan->describe.data(), (size_t)k);
    buf[k] = 0;
    if (size < n) return fail(IGN_ERR_INVALID, "buffer too small: %lld bytes needed", (long long)n);
  }
  return IGN_OK;
}
