// plan_liveness_check.cpp — stand-alone check of MPP::dead_in_last_iter as lower_plan sets it
// (ignnition_amd/csrc/plan_lower.cpp mark_dead_last; no GPU, no HIP): which MPs' last-iteration update
// nothing reads, over small plans written out as ign_plan_descs.  tests/test_plan_liveness.py builds
// this with g++, plain and under -fsanitize=address,undefined, and runs it; a non-zero exit is a failure.
#include "lower_check.h"

#include "../../ignnition_amd/csrc/plan_lower.h"

// a plan description that owns its arrays: every entity and cell at 32, every source a direct
// assignation, predict 32 -> 8 -> 1
struct Mp {
  int dst, aggr;
  std::vector<ign_source_desc> src;
};
struct Ro {
  int type;
  std::vector<int32_t> in;
  int mode = 0, adj = -1;
  std::vector<ign_dense_desc> dense;
};
struct PD {
  int n_ents = 2, n_adj = 2, n_il = 0;
  std::vector<Mp> mps;
  std::vector<Ro> ops;
  std::vector<int32_t> ro_in;
};
static ign_source_desc src(int entity, int adj, int il = -1) { return {entity, adj, il, 0, nullptr, 0, 0, nullptr}; }

// the flags of d's MPs in order, or {-1} and a FAIL line where the lowering refuses it
static std::vector<int> dead(PD& d, bool dead_last_switch = true) {
  std::vector<ign_entity_desc> ents(d.n_ents, ign_entity_desc{32, 1});
  std::vector<ign_cell_desc> cells(d.mps.size(), ign_cell_desc{32, 32});
  std::vector<ign_mp_desc> mpd;
  for (size_t m = 0; m < d.mps.size(); ++m)
    mpd.push_back({d.mps[m].dst, d.mps[m].aggr, 0, (int32_t)m, (int32_t)d.mps[m].src.size(), d.mps[m].src.data(), 0});
  std::vector<ign_readout_op_desc> opd;
  for (auto& o : d.ops)
    opd.push_back({o.type, (int32_t)o.in.size(), o.in.data(), o.mode, o.adj, (int32_t)o.dense.size(),
                   o.dense.empty() ? nullptr : o.dense.data()});
  const ign_dense_desc dense[2] = {{8, IGN_ACT_RELU, 1, 0.f}, {1, IGN_ACT_LINEAR, 1, 0.f}};
  ign_plan_desc pd{};
  pd.num_iterations = 3;
  pd.num_entities = d.n_ents;
  pd.entities = ents.data();
  pd.num_adjacencies = d.n_adj;
  pd.num_interleave = d.n_il;
  pd.num_mps = (int32_t)mpd.size();
  pd.mps = mpd.data();
  pd.num_cells = (int32_t)cells.size();
  pd.cells = cells.data();
  pd.num_readout_inputs = (int32_t)d.ro_in.size();
  pd.readout_inputs = d.ro_in.data();
  pd.num_dense = 2;
  pd.dense = dense;
  pd.num_readout_ops = (int32_t)opd.size();
  pd.readout_ops = opd.empty() ? nullptr : opd.data();
  PlanModel m;
  PlanSwitches sw;
  sw.dead_last = dead_last_switch;
  const int rc = lower_plan(&pd, sw, &m);
  if (rc) {
    printf("FAIL [%s]: lower_plan returned %d (%s)\n", g_case, rc, g_msg);
    ++g_bad;
    return {-1};
  }
  CHECK(m.dead_last == dead_last_switch);
  std::vector<int> out;
  for (const MPP& mp : m.mps) out.push_back(mp.dead_in_last_iter);
  return out;
}

// links 0, paths 1: ordered links -> paths, sum paths -> links
static PD routenet() {
  PD d;
  d.mps = {{1, IGN_AGGR_ORDERED, {src(0, 0)}}, {0, IGN_AGGR_SUM, {src(1, 1)}}};
  d.ro_in = {1};
  return d;
}

int main() {
  g_case = "routenet";   // predict reads the paths: the link update feeds only the next iteration
  {
    PD d = routenet();
    EQ(dead(d), 0, 1);
    EQ(dead(d, false), 0, 1);   // the flag is the model's; the switch only says whether it is used
  }
  g_case = "qsize";   // links 0, paths 1, nodes 2: interleave {links, nodes} -> paths, sums back to both
  {
    PD d;
    d.n_ents = 3, d.n_adj = 4, d.n_il = 2;
    d.mps = {{1, IGN_AGGR_INTERLEAVE, {src(0, 0, 0), src(2, 1, 1)}}, {0, IGN_AGGR_SUM, {src(1, 2)}}, {2, IGN_AGGR_SUM, {src(1, 3)}}};
    d.ro_in = {1};
    EQ(dead(d), 0, 1, 1);
  }
  g_case = "single entity";   // nodes -> nodes, predict on the nodes
  {
    PD d;
    d.n_ents = 1, d.n_adj = 1;
    d.mps = {{0, IGN_AGGR_SUM, {src(0, 0)}}};
    d.ro_in = {0};
    EQ(dead(d), 0);
  }
  g_case = "routenet, predict on the links";
  {
    PD d = routenet();
    d.ro_in = {0};
    EQ(dead(d), 0, 0);   // the paths feed the link update of the same iteration
  }
  g_case = "routenet, links pooled";   // sum of the links per graph times the paths' states
  {
    PD d = routenet();
    d.ops = {{IGN_RO_POOLING, {0}, IGN_POOL_SUM}, {IGN_RO_PRODUCT, {1, 2}, 0}};   // tensors 2 (graph), 3 (paths)
    d.ro_in = {3};
    EQ(dead(d), 0, 0);
  }
  g_case = "routenet, links in an unused operation";   // read is read, whatever becomes of the output
  {
    PD d = routenet();
    d.ops = {{IGN_RO_NEURAL_NETWORK, {0}, 0, -1, {{4, IGN_ACT_RELU, 1, 0.f}}}};
    EQ(dead(d), 0, 0);
  }
  g_case = "routenet, extend_adjacencies";   // reads both ends of the adjacency
  {
    PD d = routenet();
    d.ops = {{IGN_RO_EXTEND, {0, 1}, 0, 0}};   // tensors 2, 3 on adjacency 0's edges
    d.ro_in = {3};
    EQ(dead(d), 0, 0);
  }
  g_case = "two stages";   // a -> b, then b -> c in the same iteration; predict on c; then c -> a
  {
    PD d;
    d.n_ents = 3, d.n_adj = 3;
    d.mps = {{1, IGN_AGGR_SUM, {src(0, 0)}}, {2, IGN_AGGR_SUM, {src(1, 1)}}, {0, IGN_AGGR_SUM, {src(2, 2)}}};
    d.ro_in = {2};
    EQ(dead(d), 0, 0, 1);   // b is read by the second MP, c by predict, a by nothing after the last
  }
  g_case = "same destination twice";   // a -> b, c -> b: the second reads the first's b as its state
  {
    PD d;
    d.n_ents = 3;
    d.mps = {{1, IGN_AGGR_SUM, {src(0, 0)}}, {1, IGN_AGGR_SUM, {src(2, 1)}}};
    d.ro_in = {0};
    EQ(dead(d), 0, 1);
  }
  g_case = "input overwritten later";   // a -> b, then c -> a: run after the forward, the first would read the new a
  {
    PD d;
    d.n_ents = 3;
    d.mps = {{1, IGN_AGGR_SUM, {src(0, 0)}}, {0, IGN_AGGR_SUM, {src(2, 1)}}};
    d.ro_in = {0};
    EQ(dead(d), 0, 0);
    std::swap(d.mps[0], d.mps[1]);   // c -> a, then a -> b: nothing touches a after b's update
    EQ(dead(d), 0, 1);
  }
  if (g_bad) printf("plan_liveness_check: %d failed checks\n", g_bad);
  else printf("plan_liveness_check: ok\n");
  return g_bad ? 1 : 0;
}
