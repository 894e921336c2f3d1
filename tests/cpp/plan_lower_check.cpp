// plan_lower_check.cpp — stand-alone check of ignnition_amd/csrc/plan_lower.cpp (no GPU, no HIP): five
// small plans written out as ign_plan_descs.  (a) the raw parameter tensors, n_params and n_packed of
// the first two against tables worked out by hand from the 64-float alignment rule; (b) for every plan
// and readout variant, the invariants that tie the packed layout to its pack list; (c) every refusal
// of the lowering a C description can reach, by code and text; (d) train_seq_variant over its
// switches; (e) the Dropout and LayerNormalization layers of the readout stacks: the site arrays, every
// stack's seq and the gamma / beta tensors after adds in and out of stack order, and the adds'
// refusals.  tests/test_plan_lower.py builds this with g++, plain and under
// -fsanitize=address,undefined, and runs it; a non-zero exit is a failure.
#include "lower_check.h"

#include "../../ignnition_amd/csrc/plan_lower.h"

// a plan description that owns its arrays
struct Mp {
  int dst, aggr, cell;
  std::vector<ign_source_desc> src;
  int axis = 0, act = 0;
};
struct Ro {
  int type;
  std::vector<int32_t> in;
  int mode = 0, adj = -1;
  std::vector<ign_dense_desc> dense;
};
struct PD {
  int T = 2;
  std::vector<ign_entity_desc> ents;
  int n_adj = 0, n_il = 0;
  std::vector<Mp> mps;
  std::vector<ign_cell_desc> cells;
  std::vector<int32_t> ro_in;
  std::vector<ign_dense_desc> dense;
  std::vector<Ro> ops;
  int n_ents = -1, n_ops = -1;   // (the counts, where a case states them apart from the arrays)
  std::vector<ign_mp_desc> mpd;
  std::vector<ign_readout_op_desc> opd;
  ign_plan_desc d{};
  const ign_plan_desc* make() {
    mpd.clear(), opd.clear();
    for (auto& m : mps) mpd.push_back({m.dst, m.aggr, m.axis, m.cell, (int32_t)m.src.size(), m.src.data(), m.act});
    for (auto& o : ops)
      opd.push_back({o.type, (int32_t)o.in.size(), o.in.empty() ? nullptr : o.in.data(), o.mode, o.adj,
                     (int32_t)o.dense.size(), o.dense.empty() ? nullptr : o.dense.data()});
    d = ign_plan_desc{};
    d.num_iterations = T;
    d.num_entities = n_ents >= 0 ? n_ents : (int32_t)ents.size();
    d.entities = ents.data();
    d.num_adjacencies = n_adj;
    d.num_interleave = n_il;
    d.num_mps = (int32_t)mpd.size();
    d.mps = mpd.data();
    d.num_cells = (int32_t)cells.size();
    d.cells = cells.data();
    d.num_readout_inputs = (int32_t)ro_in.size();
    d.readout_inputs = ro_in.data();
    d.num_dense = (int32_t)dense.size();
    d.dense = dense.data();
    d.num_readout_ops = n_ops != -1 ? n_ops : (int32_t)opd.size();
    d.readout_ops = opd.empty() ? nullptr : opd.data();
    return &d;
  }
};
static ign_source_desc src(int entity, int adj, int il = -1) { return {entity, adj, il, 0, nullptr, 0, 0, nullptr}; }
static ign_source_desc src_net(int entity, int adj, const std::vector<int32_t>& inputs, int param_dim,
                               const std::vector<ign_dense_desc>& layers) {
  return {entity, adj, -1, (int32_t)inputs.size(), inputs.data(), param_dim, (int32_t)layers.size(), layers.data()};
}
static int lower(PD& d, PlanModel* m = nullptr, int readout_variant = 4) {
  PlanModel local;
  PlanSwitches sw;
  sw.readout_variant = readout_variant;
  return lower_plan(d.make(), sw, m ? m : &local);
}

// RouteNet-shaped: links (0) and paths (1) at H = 32; ordered links -> paths, sum paths -> links;
// predict 32 -> 256 -> 256 -> 1 selu on the paths: the fused readout
static PD routenet() {
  PD d;
  d.ents = {{32, 1}, {32, 1}};
  d.n_adj = 2;
  d.cells = {{32, 32}, {32, 32}};
  d.mps = {{1, IGN_AGGR_ORDERED, 0, {src(0, 0)}}, {0, IGN_AGGR_SUM, 1, {src(1, 1)}}};
  d.ro_in = {1};
  d.dense = {{256, IGN_ACT_SELU, 1, 0.f}, {256, IGN_ACT_SELU, 1, 0.f}, {1, IGN_ACT_LINEAR, 1, 0.f}};
  return d;
}
// Q-size-shaped: links (0), paths (1), nodes (2) at H = 16; interleave links, nodes -> paths; a sum
// with two sources (paths, nodes -> links); sum paths -> nodes; predict 16 -> 8 -> 1, the last
// layer without bias
static PD qsize() {
  PD d;
  d.ents = {{16, 1}, {16, 1}, {16, 0}};
  d.n_adj = 5, d.n_il = 2;
  d.cells = {{16, 16}, {16, 16}, {16, 16}};
  d.mps = {{1, IGN_AGGR_INTERLEAVE, 0, {src(0, 0, 0), src(2, 1, 1)}},
           {0, IGN_AGGR_SUM, 1, {src(1, 2), src(2, 3)}},
           {2, IGN_AGGR_SUM, 2, {src(1, 4)}}};
  d.ro_in = {1};
  d.dense = {{8, IGN_ACT_RELU, 1, 0.f}, {1, IGN_ACT_LINEAR, 0, 0.f}};
  return d;
}
// two entities at H = 64: the 64/64 cell's split-fp16 / split-bf16 fragments
static PD wide64() {
  PD d;
  d.ents = {{64, 2}, {64, 0}};
  d.n_adj = 2;
  d.cells = {{64, 64}, {64, 64}};
  d.mps = {{0, IGN_AGGR_SUM, 0, {src(1, 0)}}, {1, IGN_AGGR_ORDERED, 1, {src(0, 1)}}};
  d.ro_in = {0};
  d.dense = {{128, IGN_ACT_RELU, 1, 0.f}, {1, IGN_ACT_LINEAR, 1, 0.f}};
  return d;
}
// concat on axis 2 into entity 1 (H = 32): entity 0's states (16) beside the messages (16) of a network
// on [entity 2's state (16) | 24 edge parameters]: din 40, padded to 48
static const std::vector<int32_t> kNetInputs = {IGN_MSG_HS_SOURCE, IGN_MSG_EDGE_PARAMS};
static const std::vector<ign_dense_desc> kNetLayers = {{32, IGN_ACT_RELU, 1, 0.f}, {16, IGN_ACT_LINEAR, 0, 0.f}};
static PD concat2() {
  PD d;
  d.ents = {{16, 1}, {32, 1}, {16, 1}};
  d.n_adj = 2;
  d.cells = {{32, 32}};
  d.mps = {{1, IGN_AGGR_CONCAT, 0, {src(0, 0), src_net(2, 1, kNetInputs, 24, kNetLayers)}, 2}};
  d.ro_in = {1};
  d.dense = {{64, IGN_ACT_TANH, 1, 0.f}, {3, IGN_ACT_LINEAR, 1, 0.f}};
  return d;
}
// one attention MP on entity 0 (H = 32); readout: a network 32 -> 64 -> 32 (the second layer without
// bias) on the states, its rows summed per graph; predict 32 -> 16 -> 1 on the sums
static PD attention() {
  PD d;
  d.ents = {{32, 3}};
  d.n_adj = 1;
  d.cells = {{32, 32}};
  d.mps = {{0, IGN_AGGR_ATTENTION, 0, {src(0, 0)}}};
  d.ops = {{IGN_RO_NEURAL_NETWORK, {0}, 0, -1, {{64, IGN_ACT_RELU, 1, 0.f}, {32, IGN_ACT_LINEAR, 0, 0.f}}},
           {IGN_RO_POOLING, {1}, IGN_POOL_SUM}};
  d.ro_in = {2};
  d.dense = {{16, IGN_ACT_RELU, 1, 0.f}, {1, IGN_ACT_LINEAR, 1, 0.f}};
  return d;
}

// ---------------------------------------------------------------------------------------------
// (a) tables by hand.  Every tensor starts at a multiple of 64 floats: the next offset is the end of
// the tensor rounded up to 64.
struct Want { int kind, owner; long long offset; int rows, cols; };
static void tensors_are(const PlanModel& m, std::initializer_list<Want> want) {
  CHECK(m.tensors.size() == want.size());
  size_t i = 0;
  for (const Want& w : want) {
    if (i >= m.tensors.size()) break;
    const Tensor& t = m.tensors[i];
    if (t.kind != w.kind || t.owner != w.owner || t.offset != w.offset || t.rows != w.rows || t.cols != w.cols) {
      printf("FAIL [%s] tensor %zu = {%d, %d, %lld, %d, %d} want {%d, %d, %lld, %d, %d}\n", g_case, i, t.kind, t.owner,
             (long long)t.offset, t.rows, t.cols, w.kind, w.owner, w.offset, w.rows, w.cols);
      ++g_bad;
    }
    ++i;
  }
}

static void routenet_tables() {
  g_case = "routenet tables";
  PD d = routenet();
  PlanModel m;
  OK(lower(d, &m));
  // a cell at 32 / 32: kernel and recurrent kernel [32][96] = 3072 = 48 * 64 floats each, biases
  // [2][96] = 192 = 3 * 64: 6336 per cell, no padding
  // predict: W [32][256] = 8192, b 256, W [256][256] = 65536, b 256, W [256][1] = 256, b [1][1] = 1 -> 64
  tensors_are(m, {{0, 0, 0, 32, 96}, {1, 0, 3072, 32, 96}, {2, 0, 6144, 2, 96},
                  {0, 1, 6336, 32, 96}, {1, 1, 9408, 32, 96}, {2, 1, 12480, 2, 96},
                  {3, 0, 12672, 32, 256}, {4, 0, 20864, 1, 256}, {3, 1, 21120, 256, 256}, {4, 1, 86656, 1, 256},
                  {3, 2, 86912, 256, 1}, {4, 2, 87168, 1, 1}});
  CHECK(m.n_params == 87232);
  CHECK(m.fused_readout);
  // packed, per cell: W 3072, U 3072, biases [4][32] = 128, U bf16 9 * 1024 / 2 = 4608, U fp16 3072 + 64
  // = 3136, W bf16 4608: 18624 per cell, every size a multiple of 64 -> the cells end at 37248
  CHECK(m.cells[1].pk_w == 18624 && m.cells[1].pk_wbf == 32640);
  // predict layer 0 (32 -> 256): W 8192, fused bf16 12288, training bf16 12288 + fp16 8256, the
  // transposed pair 12288 + 8256 -> 37248 + 61568 = 98816
  CHECK(m.dense[0].pk_w == 37248 && m.dense[0].pk_ht == 90560 && m.dense[1].pk_w == 98816);
  // layer 1 (256 -> 256): W 65536, fused bf16 98304, the fp16 block 65536 + 64 + 32 * 256 + 64 = 73856,
  // bf16 98304 + fp16 65600, transposed 98304 + 65600 -> 98816 + 565504 = 664320; layer 2 (256 -> 1): none
  CHECK(m.dense[1].pk_h == 262656 && m.dense[1].pk_h32 == -1 && m.dense[1].pk_ht == 598720);
  // backward, per cell: U^T 3072, its fp16 form 3136, W^T 3072 = 9280 -> 682880; then W^T of
  // layer 0 (8192) and layer 1 (65536)
  CHECK(m.cells[0].pk_ut == 664320 && m.cells[1].pk_wt == 679808 && m.dense[0].pk_wt == 682880);
  CHECK(m.n_packed == 756608);
  PlanModel m5;
  OK(lower(d, &m5, 5));   // variant 5: a second fp16 block of 73856 after the first
  CHECK(m5.dense[1].pk_h32 == 262656 + 73856 && m5.n_packed == 756608 + 73856);
}

static void qsize_tables() {
  g_case = "qsize tables";
  PD d = qsize();
  PlanModel m;
  OK(lower(d, &m));
  // a cell at 16 / 16: kernels [16][48] = 768 = 12 * 64 each, biases [2][48] = 96 -> 128: 1664 per cell
  // predict: W [16][8] = 128, b 8 -> 64, W [8][1] = 8 -> 64, no bias tensor for the last layer
  tensors_are(m, {{0, 0, 0, 16, 48}, {1, 0, 768, 16, 48}, {2, 0, 1536, 2, 48},
                  {0, 1, 1664, 16, 48}, {1, 1, 2432, 16, 48}, {2, 1, 3200, 2, 48},
                  {0, 2, 3328, 16, 48}, {1, 2, 4096, 16, 48}, {2, 2, 4864, 2, 48},
                  {3, 0, 4992, 16, 8}, {4, 0, 5120, 1, 8}, {3, 1, 5184, 8, 1}});
  CHECK(m.n_params == 5248);
  CHECK(!m.fused_readout);
  // packed, per cell: W 768, U 768, biases [4][16] = 64 = 1600 (H = 16 has no bf16 / fp16 forms) -> 4800;
  // no Dense fragment (8 and 1 units); backward per cell U^T 768 + W^T 768 -> 4800 + 3 * 1536
  CHECK(m.cells[2].pk_b == 4736 && m.cells[0].pk_ut == 4800 && m.cells[2].pk_wt == 8640);
  CHECK(m.n_packed == 9408);
  CHECK(m.mps.size() == 3 && m.mps[0].sorted && !m.mps[1].sorted && m.mps[1].src.size() == 2 && m.mps[1].din == 16);
}

// ---------------------------------------------------------------------------------------------
// (b) what ties the packed layout to its pack list
struct Range { int64_t lo, hi; };
static bool disjoint_inside(std::vector<Range> r, int64_t total) {
  std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
  int64_t end = 0;
  for (auto& x : r) {
    if (x.lo < end || x.hi <= x.lo) return false;
    end = x.hi;
  }
  return end <= total;
}
// a [rows][cols] block at raw offset `at` lies in a tensor of that row width
static bool in_tensor(const PlanModel& m, int64_t at, int64_t rows, int cols) {
  for (auto& t : m.tensors)
    if (t.cols == cols && at >= t.offset && (at - t.offset) % cols == 0 && at + rows * cols <= t.offset + (int64_t)t.rows * t.cols)
      return true;
  return false;
}
static bool src_shapes_ok(const PlanModel& m, const PackJob& j) {
  const int64_t* s = j.src;
  switch (j.kind) {
    case PK_GRU: return in_tensor(m, s[0], j.a, 3 * j.b) && in_tensor(m, s[1], j.b, 3 * j.b) && in_tensor(m, s[2], 2, 3 * j.b);
    case PK_GRU_U: return s[0] < 0 && in_tensor(m, s[1], j.b, 3 * j.b) && s[2] < 0;
    case PK_GRU_B: return s[0] < 0 && s[1] < 0 && in_tensor(m, s[2], 2, 3 * j.b);
    case PK_GRU_W: case PK_W_F16: case PK_W_BF16: return in_tensor(m, s[0], j.a, 3 * j.b) && s[1] < 0 && s[2] < 0;
    case PK_U_BF16: case PK_U_F16: case PK_UT_F16: return in_tensor(m, s[0], j.a, 3 * j.a) && s[1] < 0 && s[2] < 0;
    case PK_A: case PK_DENSE_BF16: case PK_DENSE_BF16_T: return in_tensor(m, s[0], j.a, j.b) && s[1] < 0 && s[2] < 0;
    case PK_DENSE_PAD: return j.b >= j.a && in_tensor(m, s[0], j.a, j.c) && s[1] < 0 && s[2] < 0;
    case PK_DENSE_F16: return (j.c ? in_tensor(m, s[0], j.b, j.a) : in_tensor(m, s[0], j.a, j.b)) && s[1] < 0 && s[2] < 0;
    case PK_READOUT_H16: case PK_READOUT_H32:
      return in_tensor(m, s[0], j.a, j.b) && in_tensor(m, s[1], 1, j.b) && in_tensor(m, s[2], j.b, j.c);
    case PK_ATTN_VECTORS: return in_tensor(m, s[0], j.a, j.a) && in_tensor(m, s[1], j.a, j.a) && in_tensor(m, s[2], 2 * j.a, 1);
  }
  return false;
}

static void layout_invariants(const char* name, PD (*make)(), int variant) {
  char label[64];
  snprintf(label, sizeof label, "%s variant %d", name, variant);
  g_case = label;
  PD d = make();
  PlanModel m;
  OK(lower(d, &m, variant));
  // raw tensors: aligned, non-empty, disjoint, inside [0, n_params)
  std::vector<Range> tr;
  for (auto& t : m.tensors) {
    CHECK(t.offset % 64 == 0 && t.rows > 0 && t.cols > 0);
    tr.push_back({t.offset, t.offset + (int64_t)t.rows * t.cols});
  }
  CHECK(disjoint_inside(tr, m.n_params));
  // every pk_* field of the plan
  std::vector<int64_t> fields;
  for (auto& c : m.cells) {
    for (int64_t f : {c.pk_wt, c.pk_ut, c.pk_wbf, c.pk_ubf, c.pk_wh, c.pk_uh, c.pk_uth}) fields.push_back(f);
    if (c.used) fields.insert(fields.end(), {c.pk_w, c.pk_u, c.pk_b});   // (set for used cells only)
  }
  auto dense_fields = [&](const DenseP& p, bool predict2) {
    for (int64_t f : {p.pk_w, p.pk_wt, p.pk_bf, p.pk_h, p.pk_h32, p.pk_bfn, p.pk_bft, p.pk_hn, p.pk_ht}) fields.push_back(f);
    CHECK(p.pk_h32 < 0 || (variant == 5 && predict2 && p.pk_h >= 0));
    CHECK(!(variant == 5 && p.pk_h >= 0) || p.pk_h32 >= 0);
  };
  for (auto& mp : m.mps) {
    for (int64_t f : mp.pk_slice) fields.push_back(f);
    for (auto& nn : mp.nn)
      for (auto& p : nn.layers) dense_fields(p, false);
  }
  for (auto& op : m.ro_ops)
    for (auto& p : op.layers) dense_fields(p, false);
  for (size_t l = 0; l < m.dense.size(); ++l) dense_fields(m.dense[l], l == 1);
  fields.push_back(m.pk_conv);
  fields.push_back(m.pk_w12);
  // jobs: aligned, non-empty, disjoint, inside [0, n_packed); sources in tensors of the right shape
  std::vector<Range> jr;
  for (auto& j : m.packs) {
    CHECK(j.dst % 64 == 0 && j.floats > 0);
    CHECK(src_shapes_ok(m, j));
    jr.push_back({j.dst, j.dst + j.floats});
  }
  CHECK(disjoint_inside(jr, m.n_packed));
  // a PK_GRU record is followed by its U and bias records
  for (size_t i = 0; i < m.packs.size(); ++i)
    if (m.packs[i].kind == PK_GRU)
      CHECK(i + 2 < m.packs.size() && m.packs[i + 1].kind == PK_GRU_U && m.packs[i + 2].kind == PK_GRU_B);
    else if (m.packs[i].kind == PK_GRU_U)
      CHECK(i >= 1 && m.packs[i - 1].kind == PK_GRU);
    else if (m.packs[i].kind == PK_GRU_B)
      CHECK(i >= 2 && m.packs[i - 2].kind == PK_GRU);
  // fields >= 0 <-> jobs, one to one (the slots are disjoint, so no two jobs share a dst)
  size_t set = 0;
  for (int64_t f : fields) {
    if (f < 0) {
      CHECK(f == -1);
      continue;
    }
    ++set;
    size_t hits = 0;
    for (auto& j : m.packs) hits += j.dst == f;
    CHECK(hits == 1);
  }
  CHECK(set == m.packs.size());
}

static void layout_cases() {
  for (int v : {1, 2, 4, 5}) {
    layout_invariants("routenet", routenet, v);
    layout_invariants("qsize", qsize, v);
    layout_invariants("wide64", wide64, v);
    layout_invariants("concat2", concat2, v);
    layout_invariants("attention", attention, v);
  }
  g_case = "layout shapes";
  PlanModel m;
  PD w = wide64();
  OK(lower(w, &m));
  CHECK(m.cells[0].pk_wh >= 0 && m.cells[0].pk_wbf >= 0 && m.cells[0].pk_uh >= 0 && m.cells[0].pk_uth == -1);
  PD c = concat2();
  m = PlanModel();
  OK(lower(c, &m));
  CHECK(m.mps[0].feature_concat && m.mps[0].pk_slice.size() == 2 && m.mps[0].din == 32);
  EQ(m.mps[0].slice_off, 0, 16);
  const MsgNN& nn = m.mps[0].nn[1];
  CHECK(nn.din == 40 && nn.din_pad == 48 && nn.layers[0].pk_w >= 0 && nn.layers[1].pk_w >= 0);
  for (auto& j : m.packs)
    if (j.dst == nn.layers[0].pk_w) CHECK(j.kind == PK_DENSE_PAD && j.a == 40 && j.b == 48 && j.c == 32 && j.floats == 48 * 32);
  PD a = attention();
  m = PlanModel();
  OK(lower(a, &m));
  CHECK(m.attn_F == 32 && m.pk_w12 >= 0 && m.off_att >= 0 && m.ro_ops.size() == 2 && m.ro_t.size() == 3);
  CHECK(m.ro_t[2].space == RS_GRAPH && m.ro_t[2].width == 32 && m.ro_width == 32);
  CHECK(m.ro_ops[0].layers[1].off_b == -1 && m.ro_ops[0].layers[0].pk_w >= 0 && m.ro_ops[0].layers[1].pk_w >= 0);
}

// ---------------------------------------------------------------------------------------------
// (c) refusals: one line per fail(...) of lower_mps and lower_readout, in their order.  All of them
// can be reached from a C description; ign_plan_create's own "null argument" stays in engine.cpp.
static void refusals() {
  g_case = "refusals";
  const int INV = IGN_ERR_INVALID, UNS = IGN_ERR_UNSUPPORTED;
  PD d;
#define BAD(base, edit, code, sub) \
  do {                             \
    d = base();                    \
    edit;                          \
    FAILS(lower(d), code, sub);    \
  } while (0)
  BAD(routenet, d.T = 0, INV, "num_iterations must be > 0");
  BAD(routenet, d.n_ents = 0, INV, "1..8 entities supported");
  BAD(routenet, d.n_ents = 9, INV, "1..8 entities supported");
  BAD(routenet, d.ents[1].hidden_dim = 0, INV, "entity 1: hidden_state_dimension must be > 0");
  BAD(routenet, d.ents[0].feature_total = 33, INV, "entity 0: total feature size 33 exceeds hidden_state_dimension 32");
  BAD(routenet, d.mps[1].dst = 2, INV, "mp 1: bad destination");
  BAD(routenet, d.mps[0].src.clear(), INV, "mp 0: no source entities");
  BAD(routenet, d.mps[1].src.assign(5, src(1, 1)), UNS, "mp 1: more than 4 source entities");
  BAD(qsize, d.mps[0].src.pop_back(), UNS, "mp 0: interleave aggregation supports exactly 2 sources");
  BAD(concat2, d.mps[0].axis = 3, INV, "mp 0: concat_axis must be 1 or 2");
  BAD(attention, (d.mps[0].aggr = IGN_AGGR_CONVOLUTION, d.mps[0].act = 9), UNS, "mp 0: convolution activation 9");
  BAD(routenet, d.mps[0].aggr = 17, UNS, "mp 0: aggregation 17 is not lowered");
  BAD(routenet, d.mps[0].src[0].entity = -1, INV, "mp 0: bad source entity");
  BAD(routenet, d.mps[1].src[0].adjacency = 2, INV, "mp 1: bad adjacency slot");
  BAD(qsize, d.mps[0].src[1].interleave = 2, INV, "mp 0: interleave slot missing");
  static const std::vector<int32_t> in_bad = {7}, in_params = {IGN_MSG_EDGE_PARAMS}, in_none = {},
                                    in_five = {IGN_MSG_HS_SOURCE, IGN_MSG_HS_DEST, IGN_MSG_HS_SOURCE, IGN_MSG_HS_DEST, IGN_MSG_HS_SOURCE};
  static const std::vector<ign_dense_desc> units0 = {{0, IGN_ACT_RELU, 1, 0.f}}, act9 = {{16, 9, 1, 0.f}};
  BAD(concat2, d.mps[0].src[1] = src_net(2, 1, in_bad, 24, kNetLayers), UNS, "mp 0: message input 7 is not lowered");
  BAD(concat2, d.mps[0].src[1] = src_net(2, 1, in_params, 0, kNetLayers), INV, "mp 0: message input 2 has no width");
  BAD(concat2, d.mps[0].src[1] = src_net(2, 1, in_five, 0, kNetLayers), UNS, "mp 0: more than 4 message inputs");
  BAD(concat2, d.mps[0].src[1] = src_net(2, 1, in_none, 0, kNetLayers), INV, "mp 0: empty message-network input");
  BAD(concat2, d.mps[0].src[1] = src_net(2, 1, kNetInputs, 24, units0), INV, "mp 0: message layer 0 units");
  BAD(concat2, d.mps[0].src[1] = src_net(2, 1, kNetInputs, 24, act9), UNS, "mp 0: message layer activation 9");
  BAD(qsize, d.ents[2].hidden_dim = 32, INV, "mp 0: sources have different message dimensions (16 vs 32)");
  BAD(routenet, d.mps[1].cell = 2, INV, "mp 1: bad cell index");
  BAD(routenet, d.cells[0].units = 16, INV, "mp 0: cell units 16 != destination hidden dim 32");
  BAD(routenet, d.cells[1].input_dim = 16, INV, "mp 1: cell input_dim 16 != message dim 32");
  BAD(concat2, (d.ents[0].hidden_dim = 64, d.cells[0].input_dim = 80), UNS,
      "mp 0: concat slice (input 64, units 32) not instantiated");
  BAD(routenet, (d.ents[0].hidden_dim = d.ents[1].hidden_dim = 48, d.cells = {{48, 48}, {48, 48}}), UNS,
      "mp 0: GRU shape (input 48, units 48) not instantiated (16/32, 64/64)");
  BAD(routenet, (d.mps[1].aggr = IGN_AGGR_ATTENTION, d.ents[1].hidden_dim = 16, d.cells = {{32, 16}, {16, 32}}), INV,
      "mp 1: attention needs message dim 16 == destination dim 32");
  BAD(wide64, d.mps[0].aggr = IGN_AGGR_CONVOLUTION, UNS, "mp 0: attention / convolution lowered for 16 or 32 units");
  BAD(routenet, (d.mps[0].aggr = d.mps[1].aggr = IGN_AGGR_ATTENTION, d.mps[0].src[0] = src(1, 0), d.mps[1].src[0] = src(0, 1),
                 d.ents[0].hidden_dim = 16, d.cells[1] = {16, 16}),
      INV, "mp 1: the shared attention weights have width 32, this MP needs 16");
  // the readout program
  BAD(attention, d.n_ops = -2, INV, "bad readout operation list");
  BAD(attention, d.ops[1].in.clear(), INV, "readout op 1: no input");
  BAD(attention, d.ops[1].in[0] = 2, INV, "readout op 1: input tensor 2");
  BAD(routenet, (d.ops = {{IGN_RO_NEURAL_NETWORK, {0, 1}, 0, -1, {{8, IGN_ACT_RELU, 1, 0.f}}}}), UNS,
      "readout op 0: inputs on different row spaces (concat axis 1)");
  BAD(attention, d.ops[0].dense.clear(), INV, "readout op 0: no Dense layer");
  BAD(attention, d.ops[0].dense[1].units = 0, INV, "readout op 0, dense layer 1: units must be > 0");
  BAD(attention, d.ops[0].dense[0].activation = 5, UNS, "readout op 0, dense layer 0: activation 5");
  BAD(attention, d.ops[1].mode = 3, INV, "readout op 1: pooling type 3");
  BAD(attention, (d.ops[1] = {IGN_RO_PRODUCT, {0, 1}, 1}), UNS, "readout op 1: dot_product");
  BAD(attention, (d.ops[1] = {IGN_RO_PRODUCT, {1}}), INV, "readout op 1: product needs two inputs");
  BAD(attention, (d.ops[0].dense[1].units = 16, d.ops[1] = {IGN_RO_PRODUCT, {0, 1}}), INV,
      "readout op 1: product of widths 32 and 16");
  BAD(attention, (d.ops[0].dense[1].units = 1, d.ops[1] = {IGN_RO_PRODUCT, {1, 0}}), UNS,
      "readout op 1: product of widths 1 and 32");
  BAD(routenet, (d.ops = {{IGN_RO_PRODUCT, {0, 1}}}), UNS,
      "readout op 0: product of tensors on different row spaces (entity 0, entity 1)");
  BAD(routenet, (d.ops = {{IGN_RO_EXTEND, {0}, 0, 0}}), INV, "readout op 0: extend_adjacencies needs two inputs");
  BAD(routenet, (d.n_adj = 3, d.ops = {{IGN_RO_EXTEND, {0, 1}, 0, 2}}), INV,
      "readout op 0: adjacency slot 2 is not read by any message passing");
  BAD(routenet, (d.ops = {{IGN_RO_EXTEND, {1, 0}, 0, 0}}), INV,
      "readout op 0: extend_adjacencies inputs must live on the adjacency's source and destination entities");
  BAD(attention, d.ops[1].type = 4, UNS, "readout op 1: type 4");
  // predict
  BAD(routenet, d.ro_in.clear(), INV, "readout has no input");
  BAD(routenet, d.ro_in[0] = 2, INV, "readout input tensor 2");
  BAD(routenet, (d.ro_in = {1, 0}), UNS, "predict inputs on different row spaces (concat axis 1)");
  BAD(routenet, d.dense[2].units = -1, INV, "predict 0, dense layer 2: units must be > 0");
  BAD(routenet, d.dense[1].activation = -1, UNS, "predict 0, dense layer 1: activation -1");
  BAD(routenet, d.dense.clear(), INV, "readout has no Dense layer");
#undef BAD
  // the accepted forms next to them
  d = routenet();
  d.ops = {{IGN_RO_EXTEND, {0, 1}, 0, 0}};
  d.ro_in = {2, 3};
  PlanModel m;
  FAILS(lower(d, &m), IGN_OK, "");
  CHECK(m.ro_t.size() == 4 && m.ro_t[3].space == RS_ADJ && m.ro_width == 64);
}

// ---------------------------------------------------------------------------------------------
// (d) the training forward's ordered update: split-fp16 (6) only at H = 32 with the split-fp16 training
// form, the split-bf16 gate recompute and the fused backward all on; else split-bf16 (4), or f32 (2)
// where IGN_SEQ_VARIANT asks for it
static void seq_variants() {
  g_case = "train_seq_variant";
  for (int bits = 0; bits < 8; ++bits) {
    PlanModel m;
    m.train_seq_h16 = bits & 1, m.bwd_bf = bits & 2, m.bwd_fuse = bits & 4;
    CHECK(train_seq_variant(&m, 32) == (bits == 7 ? 6 : 4));
    CHECK(train_seq_variant(&m, 64) == 4);
    m.seq_variant = 4;
    CHECK(train_seq_variant(&m, 32) == 4 && train_seq_variant(&m, 64) == 4);
    m.seq_variant = 2;
    CHECK(train_seq_variant(&m, 32) == 2 && train_seq_variant(&m, 64) == 2);
  }
}

// ---------------------------------------------------------------------------------------------
// (e) Dropout and LayerNormalization layers: add_dropout / add_layernorm keep drops and norms in site
// order and every stack's seq in the architecture's order
// RouteNet's MPs; readout op 0: a network 64 -> 16 -> 8 on the path states beside themselves (two
// inputs, concatenated); predict 8 -> 12 -> 4 -> 1 on its output
static PD stacks() {
  PD d = routenet();
  d.ops = {{IGN_RO_NEURAL_NETWORK, {1, 1}, 0, -1, {{16, IGN_ACT_RELU, 1, 0.f}, {8, IGN_ACT_LINEAR, 0, 0.f}}}};
  d.ro_in = {2};
  d.dense = {{12, IGN_ACT_RELU, 1, 0.f}, {4, IGN_ACT_TANH, 0, 0.f}, {1, IGN_ACT_LINEAR, 1, 0.f}};
  return d;
}
// the fused readout behind a one-layer network on the path states
static PD fused_behind_op() {
  PD d = routenet();
  d.ops = {{IGN_RO_NEURAL_NETWORK, {1}, 0, -1, {{32, IGN_ACT_RELU, 1, 0.f}}}};
  d.ro_in = {2};
  return d;
}

// what must hold after every add
static void site_invariants(const PlanModel& m, int line) {
  std::vector<int> drop_seen(m.drops.size(), 0), norm_seen(m.norms.size(), 0);
  for (int stack = -1; stack < (int)m.ro_ops.size(); ++stack) {
    const std::vector<DenseP>* layers = stack_layers(&m, stack);
    if (!layers) {
      CHECK(!stack_seq(&m, stack) && m.ro_ops[stack].seq.empty());
      continue;
    }
    const std::vector<StackLayer>& seq = *stack_seq(&m, stack);
    const int L = (int)layers->size();
    int l = 0;   // the Dense layer the next entries stand in front of
    std::vector<std::pair<int, int64_t>> want;   // the stack's tensors: (kind, offset)
    for (const StackLayer& e : seq) {
      const int units = l < L ? (*layers)[l].in : layers->back().out;
      if (e.kind == SL_DENSE) {
        CHECK(e.idx == l && l < L);   // each Dense index once, ascending
        if (l >= L) return;
        want.push_back({stack < 0 ? 3 : 11, (*layers)[l].off_w});
        if ((*layers)[l].use_bias) want.push_back({stack < 0 ? 4 : 12, (*layers)[l].off_b});
        ++l;
      } else if (e.kind == SL_DROPOUT) {
        CHECK(e.idx >= 0 && e.idx < (int)m.drops.size());
        if (e.idx < 0 || e.idx >= (int)m.drops.size()) return;
        const DropSite& s = m.drops[e.idx];
        ++drop_seen[e.idx];
        CHECK(s.stack == stack && s.before == l && s.units == units && s.rate > 0.f && s.scale == 1.f / (1.f - s.rate));
      } else {
        CHECK(e.kind == SL_LAYERNORM && e.idx >= 0 && e.idx < (int)m.norms.size());
        if (e.kind != SL_LAYERNORM || e.idx < 0 || e.idx >= (int)m.norms.size()) return;
        const NormSite& s = m.norms[e.idx];
        ++norm_seen[e.idx];
        CHECK(s.stack == stack && s.before == l && s.units == units);
        CHECK((s.off_gamma >= 0) == s.scale && (s.off_beta >= 0) == s.center);
        if (s.scale) want.push_back({13, s.off_gamma});
        if (s.center) want.push_back({14, s.off_beta});
      }
    }
    CHECK(l == L);
    // gamma / beta directly in front of the kernel of the Dense layer they precede, in seq order
    size_t t = 0;
    while (t < m.tensors.size() && m.tensors[t].offset != want[0].second) ++t;
    CHECK(t + want.size() <= m.tensors.size());
    for (size_t i = 0; i < want.size() && t + i < m.tensors.size(); ++i) {
      const Tensor& x = m.tensors[t + i];
      CHECK(x.kind == want[i].first && x.offset == want[i].second);
      if (x.kind == 13 || x.kind == 14) CHECK(x.rows == 1 && x.cols == m.norms[x.owner].units && (x.kind == 13 ? m.norms[x.owner].off_gamma : m.norms[x.owner].off_beta) == x.offset);
    }
  }
  // every site in exactly one seq (of the stack it names: checked above), the arrays in site order
  for (int n : drop_seen) CHECK(n == 1);
  for (int n : norm_seen) CHECK(n == 1);
  auto key = [](int stack, int before) { return std::make_pair(stack < 0 ? 1 << 30 : stack, before); };
  for (size_t i = 1; i < m.drops.size(); ++i) CHECK(key(m.drops[i - 1].stack, m.drops[i - 1].before) <= key(m.drops[i].stack, m.drops[i].before));
  for (size_t i = 1; i < m.norms.size(); ++i) CHECK(key(m.norms[i - 1].stack, m.norms[i - 1].before) <= key(m.norms[i].stack, m.norms[i].before));
  if (g_bad) printf("  (site_invariants called from line %d)\n", line);
}
// a Dropout changes neither layout; a LayerNormalization on a readout operation leaves fused_readout alone
static bool same_layouts(const PlanModel& a, const PlanModel& b) {
  bool same = a.n_params == b.n_params && a.n_packed == b.n_packed && a.tensors.size() == b.tensors.size() &&
              a.packs.size() == b.packs.size() && a.fused_readout == b.fused_readout;
  for (size_t i = 0; same && i < a.tensors.size(); ++i) {
    const Tensor &x = a.tensors[i], &y = b.tensors[i];
    same = x.kind == y.kind && x.owner == y.owner && x.offset == y.offset && x.rows == y.rows && x.cols == y.cols;
  }
  for (size_t i = 0; same && i < a.packs.size(); ++i) {
    const PackJob &x = a.packs[i], &y = b.packs[i];
    same = x.kind == y.kind && x.src[0] == y.src[0] && x.src[1] == y.src[1] && x.src[2] == y.src[2] && x.dst == y.dst &&
           x.a == y.a && x.b == y.b && x.c == y.c && x.floats == y.floats;
  }
  return same;
}
static std::vector<int> kinds(const std::vector<StackLayer>& seq) {
  std::vector<int> k;
  for (auto& e : seq) k.push_back(e.kind);
  return k;
}
#define DROPOUT(m, stack, before, rate, seed)                  \
  do {                                                         \
    const PlanModel was_ = m;                                  \
    OK(add_dropout(&m, stack, before, rate, seed));            \
    CHECK(same_layouts(was_, m));                              \
    site_invariants(m, __LINE__);                              \
  } while (0)
#define LAYERNORM(m, stack, before, eps, center, scale)              \
  do {                                                               \
    OK(add_layernorm(&m, stack, before, eps, center, scale));        \
    site_invariants(m, __LINE__);                                    \
  } while (0)

static void sites_in_call_order() {
  g_case = "sites: call order";
  const int D = SL_DENSE, DO = SL_DROPOUT, LN = SL_LAYERNORM;
  PD d = stacks();
  PlanModel m;
  OK(lower(d, &m));
  site_invariants(m, __LINE__);
  EQ(kinds(m.seq), D, D, D);
  EQ(kinds(m.ro_ops[0].seq), D, D);
  LAYERNORM(m, -1, 1, 1e-3f, 1, 1);
  DROPOUT(m, -1, 1, 0.5f, 3);
  EQ(kinds(m.seq), D, LN, DO, D, D);
  CHECK(site_order(&m, -1, SL_LAYERNORM, 0) == 0 && site_order(&m, -1, SL_DROPOUT, 0) == 1);
  PlanModel r;
  OK(lower(d, &r));
  DROPOUT(r, -1, 1, 0.5f, 3);
  LAYERNORM(r, -1, 1, 1e-3f, 1, 1);
  EQ(kinds(r.seq), D, DO, LN, D, D);
  CHECK(site_order(&r, -1, SL_LAYERNORM, 0) == 1 && site_order(&r, -1, SL_DROPOUT, 0) == 0);
  // the layouts do not depend on where the Dropout stands
  CHECK(same_layouts(m, r) && m.norms[0].units == 12 && m.drops[0].units == 12);
}

static void sites_out_of_stack_order() {
  g_case = "sites: out of stack order";
  const int D = SL_DENSE, DO = SL_DROPOUT, LN = SL_LAYERNORM;
  PD d = stacks();
  PlanModel m;
  OK(lower(d, &m));
  // predict first, then readout op 0, then predict again in front of an earlier layer
  DROPOUT(m, -1, 2, 0.25f, 7);
  LAYERNORM(m, -1, 2, 1e-3f, 1, 0);
  DROPOUT(m, 0, 1, 0.5f, 9);
  LAYERNORM(m, 0, 0, 1e-5f, 0, 1);   // in front of layer 0 of the two-input operation: the concatenated width
  DROPOUT(m, -1, 0, 0.125f, 11);
  LAYERNORM(m, -1, 1, 1e-2f, 1, 1);
  CHECK(m.drops.size() == 3 && m.norms.size() == 3);
  if (m.drops.size() != 3 || m.norms.size() != 3) return;
  // today's site order: readout operations in order, then predict; by position
  CHECK(m.drops[0].stack == 0 && m.drops[0].before == 1 && m.drops[0].seed == 9 && m.drops[0].rate == 0.5f && m.drops[0].units == 16);
  CHECK(m.drops[1].stack == -1 && m.drops[1].before == 0 && m.drops[1].seed == 11 && m.drops[1].units == 8);
  CHECK(m.drops[2].stack == -1 && m.drops[2].before == 2 && m.drops[2].seed == 7 && m.drops[2].units == 4);
  CHECK(m.norms[0].stack == 0 && m.norms[0].before == 0 && m.norms[0].epsilon == 1e-5f && m.norms[0].units == 64 && !m.norms[0].center);
  CHECK(m.norms[1].stack == -1 && m.norms[1].before == 1 && m.norms[1].epsilon == 1e-2f && m.norms[1].units == 12);
  CHECK(m.norms[2].stack == -1 && m.norms[2].before == 2 && !m.norms[2].scale && m.norms[2].units == 4);
  EQ(kinds(m.ro_ops[0].seq), LN, D, DO, D);
  EQ(kinds(m.seq), DO, D, LN, D, DO, LN, D);
  if (m.seq.size() != 7 || m.ro_ops[0].seq.size() != 4) return;
  CHECK(m.ro_ops[0].seq[0].idx == 0 && m.ro_ops[0].seq[2].idx == 0);
  CHECK(m.seq[0].idx == 1 && m.seq[2].idx == 1 && m.seq[4].idx == 2 && m.seq[5].idx == 2);
  // a second layer in front of the same Dense layer goes behind the first, in both lists
  DROPOUT(m, 0, 1, 0.75f, 13);
  CHECK(m.drops.size() == 4 && m.drops[1].seed == 13 && m.drops[1].stack == 0);
  EQ(kinds(m.ro_ops[0].seq), LN, D, DO, DO, D);
  CHECK(m.ro_ops[0].seq[2].idx == 0 && m.ro_ops[0].seq[3].idx == 1 && m.seq[0].idx == 2 && m.seq[4].idx == 3);
  // the tensors, by hand: readout op 0 is gamma [1][64] (no beta), W [64][16], b, W [16][8]; predict is
  // W [8][12], b, gamma and beta [1][12], W [12][4], beta [1][4] (no gamma), W [4][1], b
  const int64_t base = 2 * 6336;
  tensors_are(m, {{0, 0, 0, 32, 96}, {1, 0, 3072, 32, 96}, {2, 0, 6144, 2, 96},
                  {0, 1, 6336, 32, 96}, {1, 1, 9408, 32, 96}, {2, 1, 12480, 2, 96},
                  {13, 0, base, 1, 64}, {11, 0, base + 64, 64, 16}, {12, 0, base + 1088, 1, 16}, {11, 1, base + 1152, 16, 8},
                  {3, 0, base + 1280, 8, 12}, {4, 0, base + 1408, 1, 12}, {13, 1, base + 1472, 1, 12}, {14, 1, base + 1536, 1, 12},
                  {3, 1, base + 1600, 12, 4}, {14, 2, base + 1664, 1, 4}, {3, 2, base + 1728, 4, 1}, {4, 2, base + 1792, 1, 1}});
  CHECK(m.n_params == base + 1856);
}

static void sites_after_the_last_layer() {
  g_case = "sites: after the last layer";
  const int D = SL_DENSE, DO = SL_DROPOUT, LN = SL_LAYERNORM;
  PD d = stacks();
  PlanModel m;
  OK(lower(d, &m));
  LAYERNORM(m, -1, 3, 1e-3f, 1, 1);
  DROPOUT(m, -1, 3, 0.5f, 1);
  DROPOUT(m, 0, 2, 0.5f, 2);
  LAYERNORM(m, 0, 2, 1e-3f, 1, 1);
  EQ(kinds(m.seq), D, D, D, LN, DO);
  EQ(kinds(m.ro_ops[0].seq), D, D, DO, LN);
  CHECK(m.norms.size() == 2 && m.drops.size() == 2);
  if (m.norms.size() != 2 || m.drops.size() != 2) return;
  // the stack's output width
  CHECK(m.norms[0].stack == 0 && m.norms[0].units == 8 && m.drops[0].stack == 0 && m.drops[0].units == 8);
  CHECK(m.norms[1].stack == -1 && m.norms[1].units == 1 && m.drops[1].stack == -1 && m.drops[1].units == 1);
  // its gamma / beta close the stack's tensors
  const Tensor& last = m.tensors.back();
  CHECK(last.kind == 14 && last.owner == 1 && last.offset == m.norms[1].off_beta);
}

static void sites_and_the_fused_readout() {
  g_case = "sites: fused readout";
  PD d = fused_behind_op();
  PlanModel m;
  OK(lower(d, &m));
  CHECK(m.fused_readout);
  DROPOUT(m, -1, 1, 0.5f, 0);   // (same_layouts: fused_readout stays)
  DROPOUT(m, 0, 0, 0.5f, 0);
  const PlanModel was = m;
  LAYERNORM(m, 0, 1, 1e-3f, 1, 1);   // on a readout operation: left alone
  CHECK(m.fused_readout && m.n_params == was.n_params + 128 && m.tensors.size() == was.tensors.size() + 2);
  LAYERNORM(m, -1, 0, 1e-3f, 1, 1);   // on predict: cleared, and the fused fp16 blocks leave the packed layout
  CHECK(!m.fused_readout && m.dense[1].pk_h == -1 && m.n_packed < was.n_packed);
}

static void site_refusals() {
  g_case = "sites: refusals";
  PD d = attention();   // op 0: a network of two layers, op 1: pooling; predict: two layers
  PlanModel m;
  OK(lower(d, &m));
  const PlanModel was = m;
#define REFUSES(e, text)                 \
  do {                                   \
    FAILS(e, IGN_ERR_INVALID, text);     \
    CHECK(strcmp(g_msg, text) == 0);     \
  } while (0)
  REFUSES(add_dropout(&m, 1, 0, 0.5f, 0),
          "ign_plan_add_dropout: stack 1 is neither -1 (predict) nor a readout neural_network operation");
  REFUSES(add_layernorm(&m, 1, 0, 1e-3f, 1, 1),
          "ign_plan_add_layernorm: stack 1 is neither -1 (predict) nor a readout neural_network operation");
  REFUSES(add_dropout(&m, 2, 0, 0.5f, 0),
          "ign_plan_add_dropout: stack 2 is neither -1 (predict) nor a readout neural_network operation");
  REFUSES(add_layernorm(&m, -2, 0, 1e-3f, 1, 1),
          "ign_plan_add_layernorm: stack -2 is neither -1 (predict) nor a readout neural_network operation");
  REFUSES(add_dropout(&m, -1, -1, 0.5f, 0), "ign_plan_add_dropout: before_layer -1 outside 0..2");
  REFUSES(add_dropout(&m, 0, 3, 0.5f, 0), "ign_plan_add_dropout: before_layer 3 outside 0..2");
  REFUSES(add_layernorm(&m, 0, -1, 1e-3f, 1, 1), "ign_plan_add_layernorm: before_layer -1 outside 0..2");
  REFUSES(add_layernorm(&m, -1, 3, 1e-3f, 1, 1), "ign_plan_add_layernorm: before_layer 3 outside 0..2");
  REFUSES(add_dropout(&m, -1, 0, 1.0f, 0), "Dropout rate must be in [0, 1), got 1");
  REFUSES(add_dropout(&m, -1, 0, -0.1f, 0), "Dropout rate must be in [0, 1), got -0.1");
  REFUSES(add_layernorm(&m, -1, 0, -1.f, 1, 1), "LayerNormalization epsilon must be >= 0, got -1");
  // the checks come in that order: a bad stack is named before a bad rate
  REFUSES(add_dropout(&m, 1, 9, 2.f, 0),
          "ign_plan_add_dropout: stack 1 is neither -1 (predict) nor a readout neural_network operation");
#undef REFUSES
  // nothing was added by any of them, and a rate of 0 is no layer
  OK(add_dropout(&m, -1, 0, 0.f, 5));
  OK(add_dropout(&m, 0, 2, 0.f, 5));
  CHECK(m.drops.empty() && m.norms.empty() && m.seq.size() == 2 && m.ro_ops[0].seq.size() == 2 && m.ro_ops[1].seq.empty());
  CHECK(same_layouts(was, m));
  site_invariants(m, __LINE__);
}

int main() {
  routenet_tables();
  qsize_tables();
  layout_cases();
  refusals();
  seq_variants();
  sites_in_call_order();
  sites_out_of_stack_order();
  sites_after_the_last_layer();
  sites_and_the_fused_readout();
  site_refusals();
  if (g_bad) printf("%d check(s) failed\n", g_bad);
  else printf("plan_lower_check: ok\n");
  return g_bad ? 1 : 0;
}
