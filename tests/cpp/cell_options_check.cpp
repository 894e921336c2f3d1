// cell_options_check.cpp — stand-alone check of plan_lower.cpp's set_cell_options (no GPU, no HIP): on a
// RouteNet-shaped and a 64-wide plan, what the options do to the parameter layout (the bias tensor
// [2][3H], [3H] or absent), to pack_gru's mode, and to the split fragments whose absence takes a cell
// off the resident, split and fused paths; a cell given the Keras defaults stays the plan it was; and
// the refusals.  tests/test_gru_options_host.py builds this with g++, plain and under
// -fsanitize=address,undefined, and runs it; a non-zero exit is a failure.
#include "lower_check.h"

#include "../../ignnition_amd/csrc/plan_lower.h"

struct PD {
  std::vector<ign_entity_desc> ents;
  std::vector<ign_source_desc> s0, s1;
  std::vector<ign_mp_desc> mps;
  std::vector<ign_cell_desc> cells;
  std::vector<int32_t> ro_in = {1};
  std::vector<ign_dense_desc> dense = {{256, IGN_ACT_SELU, 1, 0.f}, {256, IGN_ACT_SELU, 1, 0.f}, {1, IGN_ACT_LINEAR, 1, 0.f}};
  ign_plan_desc d{};
  // links (0) and paths (1) at width H: ordered links -> paths (cell 0), sum paths -> links (cell 1)
  explicit PD(int H) {
    ents = {{H, 1}, {H, 1}};
    s0 = {{0, 0, -1, 0, nullptr, 0, 0, nullptr}};
    s1 = {{1, 1, -1, 0, nullptr, 0, 0, nullptr}};
    mps = {{1, IGN_AGGR_ORDERED, 0, 0, 1, s0.data(), 0}, {0, IGN_AGGR_SUM, 0, 1, 1, s1.data(), 0}};
    cells = {{H, H}, {H, H}};
    d.num_iterations = 2;
    d.num_entities = 2;
    d.entities = ents.data();
    d.num_adjacencies = 2;
    d.num_mps = 2;
    d.mps = mps.data();
    d.num_cells = 2;
    d.cells = cells.data();
    d.num_readout_inputs = 1;
    d.readout_inputs = ro_in.data();
    d.num_dense = 3;
    d.dense = dense.data();
  }
};

static const Tensor* bias_of(const PlanModel& m, int cell) {
  for (const Tensor& t : m.tensors)
    if (t.kind == 2 && t.owner == cell) return &t;
  return nullptr;
}
static const PackJob* gru_job(const PlanModel& m, int cell) {
  for (const PackJob& j : m.packs)
    if (j.kind == PK_GRU && j.dst == m.cells[cell].pk_w) return &j;
  return nullptr;
}
static bool has_split(const CellP& c) {
  return c.pk_ubf >= 0 || c.pk_uh >= 0 || c.pk_wbf >= 0 || c.pk_wh >= 0 || c.pk_uth >= 0;
}
// every slot of [0, n_packed) is written by exactly the jobs, without overlap
static void packs_cover(const PlanModel& m) {
  int64_t covered = 0;
  for (const PackJob& j : m.packs) {
    CHECK(j.dst >= 0 && j.dst + j.floats <= m.n_packed);
    covered += j.floats;
  }
  CHECK(covered <= m.n_packed);
}

static void options(int H) {
  PD d(H);
  PlanModel base, m;
  OK(lower_plan(&d.d, PlanSwitches(), &base));
  OK(lower_plan(&d.d, PlanSwitches(), &m));
  // the default plan: both cells on the fast paths' fragments, bias [2][3H], pack mode 0
  for (int c = 0; c < 2; ++c) {
    CHECK(base.cells[c].is_default() && has_split(base.cells[c]));
    CHECK(bias_of(base, c) && bias_of(base, c)->rows == 2 && bias_of(base, c)->cols == 3 * H);
    CHECK(gru_job(base, c) && gru_job(base, c)->c == 0);
  }
  // the Keras defaults written out: the same plan, tensor for tensor and job for job
  const ign_cell_options dflt{IGN_ACT_TANH, IGN_ACT_SIGMOID, 1, 1};
  OK(set_cell_options(&m, 0, &dflt));
  OK(set_cell_options(&m, 1, &dflt));
  CHECK(m.n_params == base.n_params && m.n_packed == base.n_packed && m.tensors.size() == base.tensors.size() &&
        m.packs.size() == base.packs.size());
  for (size_t i = 0; i < m.tensors.size() && i < base.tensors.size(); ++i)
    CHECK(m.tensors[i].kind == base.tensors[i].kind && m.tensors[i].offset == base.tensors[i].offset &&
          m.tensors[i].rows == base.tensors[i].rows && m.tensors[i].cols == base.tensors[i].cols);
  for (size_t i = 0; i < m.packs.size() && i < base.packs.size(); ++i)
    CHECK(m.packs[i].kind == base.packs[i].kind && m.packs[i].dst == base.packs[i].dst && m.packs[i].c == base.packs[i].c &&
          m.packs[i].floats == base.packs[i].floats);
  // a relu candidate on the path cell: the bias tensor stays [2][3H], the pack is unscaled with both bias
  // rows, and no split fragment is left (resident_plan_shape needs pk_uh / pk_wbf of MP 0's cell; the
  // split sequence variants pk_ubf / pk_uh; the fused ordered backward's split recompute pk_uth); the
  // backward's pack_a fragments are kept
  const ign_cell_options relu{IGN_ACT_RELU, IGN_ACT_SIGMOID, 1, 1};
  OK(set_cell_options(&m, 0, &relu));
  CHECK(!m.cells[0].is_default() && m.cells[0].act == IGN_ACT_RELU && !has_split(m.cells[0]));
  CHECK(m.cells[0].pk_w >= 0 && m.cells[0].pk_u >= 0 && m.cells[0].pk_b >= 0 && m.cells[0].pk_ut >= 0 && m.cells[0].pk_wt >= 0);
  CHECK(bias_of(m, 0) && bias_of(m, 0)->rows == 2 && bias_of(m, 0)->cols == 3 * H);
  CHECK(gru_job(m, 0) && gru_job(m, 0)->c == (kPackGruRaw | 2));
  CHECK(m.cells[1].is_default() && has_split(m.cells[1]) && gru_job(m, 1) && gru_job(m, 1)->c == 0);   // the link cell: untouched
  CHECK(m.n_params == base.n_params && m.n_packed < base.n_packed);
  packs_cover(m);
  // reset_after = 0, the "v1" cell: bias [3H], the unscaled pack with one bias row, no split fragment
  const ign_cell_options v1{IGN_ACT_TANH, IGN_ACT_SIGMOID, 1, 0};
  OK(set_cell_options(&m, 0, &v1));
  CHECK(!m.cells[0].is_default() && !m.cells[0].reset_after && m.cells[0].act == IGN_ACT_TANH && !has_split(m.cells[0]));
  CHECK(bias_of(m, 0) && bias_of(m, 0)->rows == 1 && bias_of(m, 0)->cols == 3 * H);
  CHECK(gru_job(m, 0) && gru_job(m, 0)->c == (kPackGruRaw | 1) && m.cells[0].pk_ut >= 0 && m.cells[0].pk_wt >= 0);
  CHECK(m.n_params < base.n_params && m.any_cell_options);
  packs_cover(m);
  // use_bias false and other functions on the link cell: no bias tensor, a bias block of zeros, and no
  // split fragment: sum_gru_g32 (its split-bf16 step and its fused projection) needs pk_wbf / pk_ubf
  const ign_cell_options nb{IGN_ACT_RELU, IGN_ACT_HARD_SIGMOID, 0, 1};
  OK(set_cell_options(&m, 1, &nb));
  CHECK(!bias_of(m, 1) && m.cells[1].off_b == -1 && m.cells[1].act == IGN_ACT_RELU && m.cells[1].ract == IGN_ACT_HARD_SIGMOID);
  CHECK(!has_split(m.cells[1]) && gru_job(m, 1) && gru_job(m, 1)->c == kPackGruRaw && gru_job(m, 1)->src[2] == -1);
  CHECK(m.tensors.size() + 1 == base.tensors.size());
  packs_cover(m);
  // back to the defaults: the plan it was
  OK(set_cell_options(&m, 0, &dflt));
  OK(set_cell_options(&m, 1, &dflt));
  CHECK(m.n_params == base.n_params && m.n_packed == base.n_packed && has_split(m.cells[0]) && has_split(m.cells[1]) &&
        !m.any_cell_options);
  // refusals
  FAILS(set_cell_options(&m, 2, &dflt), IGN_ERR_INVALID, "ign_plan_set_cell_options: cell 2 outside 0..1");
  FAILS(set_cell_options(&m, -1, &dflt), IGN_ERR_INVALID, "ign_plan_set_cell_options: cell -1 outside 0..1");
  FAILS(set_cell_options(&m, 0, nullptr), IGN_ERR_INVALID, "null options");
  const ign_cell_options bad_a{10, IGN_ACT_SIGMOID, 1, 1}, bad_r{IGN_ACT_TANH, -1, 1, 1};
  FAILS(set_cell_options(&m, 0, &bad_a), IGN_ERR_INVALID, "activation code 10");
  FAILS(set_cell_options(&m, 0, &bad_r), IGN_ERR_INVALID, "activation code -1");
  CHECK(m.cells[0].is_default());   // a refused call changes nothing
}

int main() {
  g_case = "H 32";
  options(32);
  g_case = "H 64";
  options(64);
  g_case = "H 16";
  {   // no split fragment exists at H 16: the options still change the bias tensor and the pack mode
    PD d(16);
    PlanModel m;
    int rc = lower_plan(&d.d, PlanSwitches(), &m);
    const ign_cell_options nb{IGN_ACT_TANH, IGN_ACT_SIGMOID, 0, 1};
    if (!rc) rc = set_cell_options(&m, 1, &nb);
    CHECK(rc == 0 && !bias_of(m, 1) && gru_job(m, 1) && gru_job(m, 1)->c == kPackGruRaw);
  }
  if (g_bad) printf("cell_options_check: %d failure(s)\n", g_bad);
  else printf("cell_options_check: ok\n");
  return g_bad ? 1 : 0;
}
