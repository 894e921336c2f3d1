// batch_lower.h — the host-side lowering of a batch: from an ign_batch_desc and the plan's MPs to the
// index tables the kernels walk.  Pure host code (no HIP header, no device or pool call), so it runs
// and is checked on a CPU (tests/cpp/batch_lower_check.cpp); engine.cpp uploads what it returns.
// Every function returns IGN_OK or an error set through ign::fail.
#pragma once
#include "host_types.h"

namespace ign {

// rows and offsets of the whole batch, and the desc's index arrays at their own width
struct BatchShape {
  const ign_batch_desc* d = nullptr;
  int G = 0;
  std::vector<int64_t> rows;                    // per entity (owned rows)
  std::vector<int64_t> halo;                    // per entity: peer rows after the owned ones (§8e)
  std::vector<std::vector<int64_t>> row_off;    // [entity][graph]
  std::vector<hvec<int64_t>> eoff, ioff;        // [adjacency | interleave slot][graph + 1]
  std::vector<IdxArr> asrc, adst, aseq, ilx;    // ABI 13: int32 or int64
};
int lower_batch_shape(int n_ents, int n_adj, int n_il, const std::vector<MPP>& mps, const ign_batch_desc* d,
                      BatchShape* out);

// messages of one MP: (dst row, position, code), in source order then edge order; flen = final_len per
// destination row
struct MsgLists {
  hvec<int32_t> mdst;   // rows < IGN_ROW_MASK
  hvec<int32_t> mpos;   // < total_slots (checked)
  hvec<uint32_t> mcode;
  hvec<int64_t> flen;
  int64_t tot = 0;      // edges of the MP's adjacencies
};
int lower_messages(const MPP& mp, const BatchShape& sh, MsgLists* out);

// message network of source s (GM:440-475): global source / destination row of every edge
int lower_edge_rows(const MPP& mp, size_t mi, int s, const BatchShape& sh, hvec<int32_t>* es, hvec<int32_t>* ed);

// table rows of source s: its entity's rows, or its edges under a message network
int64_t source_rows(const MPP& mp, int s, const BatchShape& sh);

struct OrderedTables {
  hvec<int32_t> order, len, step_ptr, multi_ptr, hdr;
  hvec<uint32_t> step_code, multi_rows;
  std::vector<int64_t> src_off, src_rows;   // first table row / rows of each source
  int64_t zero_row = 0, n_multi = 0, n_steps = 0, n_msgs = 0, wave_steps = 0;
  double flops = 0, bytes = 0;              // algorithmic, per launch
};
int lower_ordered(const MPP& mp, int H, const BatchShape& sh, const MsgLists& ml, BuildMarks& bm, OrderedTables* out);

struct SumCsr {
  hvec<int32_t> order, ptr, csr_pos;   // csr_pos (attention only): message -> CSR slot
  hvec<uint32_t> msrc;
  int64_t n_interior = 0;              // order[0, n_interior) reads no halo row
  bool halo = false;                   // a source entity has halo rows
};
void lower_sum_csr(const MPP& mp, const BatchShape& sh, const MsgLists& ml, BuildMarks& bm, SumCsr* out);

struct AttnTables {
  hvec<int32_t> group_ptr, group_empty, cell_dst, cell_ptr, cell_msgs;
  int64_t n_groups = 0, n_cells = 0;
};
void lower_attention(const MPP& mp, const BatchShape& sh, const MsgLists& ml, const SumCsr& csr, AttnTables* out);

// how a sum MP aggregates: windowed (sum_window 1) or segmented for order positions [0, n_seg), else
// neither (both flags false: the GRU step's lane walk over the MP's own CSR)
struct SumAgg {
  bool window = false, seg = false;
  int64_t n_seg = 0, n_win_wg = 0;
  hvec<int64_t> wg;
  hvec<int32_t> wdst, wptr, wsrc, id_ptr;
  hvec<uint32_t> id_src;
};
int lower_sum_agg(const MPP& mp, size_t mi, int sum_window, const BatchShape& sh, const MsgLists& ml,
                  const SumCsr& csr, SumAgg* out);

// ---------------------------------------------------------------------------------------------
// The graph-resident forward's per-graph tables (resident.hip), K graphs per workgroup.
constexpr int kResMaxSrc = 2;                                     // kernels.h: kResidentMaxSrc
enum { kResAllLds = 0, kResPathGlobal = 1, kResPathCsrGlobal = 2 };   // kernels.h: IGN_RES_* forms
struct ResidentParams {
  int path = -1, n_src = 0;            // the ordered MP's destination entity and its S sources
  int src_ent[kResMaxSrc] = {-1, -1};
  int T = 0, sum_window = -1;
  bool path_global_ok = true;          // plan->resident_pg
  bool force_path_global = false;      // plan->resident_path_global
  bool dead_last[kResMaxSrc] = {false, false};   // source s's last sum update is left out (the cost model)
  // the kernel's limits (kernels.h)
  int max_tiles = 0, state_stride = 0, table_stride = 0;
  size_t max_dyn_lds = 0;
  std::vector<int> feature_total;      // per entity
};
// the host tables of the ordered MP and of source s's sum MP (the batch's MPB host copies)
struct ResOrderedIn {
  const hvec<int32_t>&h_order, &h_len, &h_step_ptr;
  const hvec<uint32_t>& h_step_code;
  const std::vector<int64_t>& src_off;
  int64_t zero_row, n_multi, n_steps;
  double flops, bytes;
};
struct ResSumIn {
  const hvec<int32_t>&h_order, &h_msg_ptr;
  const hvec<uint32_t>& h_msg_src;
  double flops, bytes;
};
struct ResidentTables {
  bool eligible = false;
  int K = 0, G = 0;                    // graphs per workgroup, workgroups
  int form = 0, train_form = 0;
  size_t lds[3] = {0, 0, 0};           // dynamic LDS of the largest group, per form
  std::vector<int64_t> path_off, src_off[kResMaxSrc], urow_off;
  hvec<int32_t> ptile_off, hdr, hsb, lmsg_off, lmsg_ptr, lnseg, gorder, lcode_off;
  hvec<uint16_t> lmsg_src, lorder, lcode;
  ign_resident_info_t info{};          // the cost model of one launch as rp.dead_last says
  ign_resident_info_t info_full{};     // ... with every update (the training forward's launch)
};
struct BatchRows {   // views of the batch's G, row_off, rows, halo (BatchShape's, or the ign_batch's copies)
  int G;
  const std::vector<std::vector<int64_t>>& row_off;
  const std::vector<int64_t>&rows, &halo;
};
// out->eligible false: the batch takes the per-MP launches
void lower_resident(const ResidentParams& rp, int K, const BatchRows& b, const ResOrderedIn& ma,
                    const std::vector<ResSumIn>& sums, ResidentTables* out);

}  // namespace ign
