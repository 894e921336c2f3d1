// batch_lower_check.cpp — stand-alone check of ignnition_amd/csrc/batch_lower.cpp (no GPU, no HIP):
// tiny batches whose tables are written out by hand.  tests/test_batch_lower.py builds it with g++,
// plain and under -fsanitize=address,undefined, and runs it; a non-zero exit is a failure.
// Exempt (they need 2^29 rows / 2^31 slots): "too many rows", "sequences too long", "MP too large",
// "too many edges for a message network".
#include "lower_check.h"

// ---------------------------------------------------------------------------------------------
// ordered MP: entity 0 -> entity 1, G = 2, destination lengths {2, 1} and {3}
static Desc ordered_desc(bool hole_and_multi) {
  std::vector<Edge> g1 = {{1, 0, 0}, {0, 0, 1}, {1, 0, 2}};
  if (hole_and_multi) g1 = {{1, 0, 0}, {0, 0, 2}, {1, 0, 2}};   // position 1 skipped, two messages on position 2
  return Desc(2, 2, {3, 2, 2, 1}, {{{{0, 0, 0}, {1, 0, 1}, {2, 1, 0}}, g1}});
}
static void ordered_case(int ib) {
  Desc ds = ordered_desc(false);
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_ORDERED, true, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  EQ(sh.rows, 5, 3);
  EQ(sh.row_off[0], 0, 3, 5);
  EQ(sh.row_off[1], 0, 2, 3);
  EQ(sh.eoff[0], 0, 3, 6);
  EQ(ml.mdst, 0, 0, 1, 2, 2, 2);
  EQ(ml.mpos, 0, 1, 0, 0, 1, 2);
  EQ(ml.mcode, 0, 1, 2, 4, 3, 4);
  EQ(ml.flen, 2, 1, 3);
  CHECK(ml.tot == 6);
  OrderedTables t;
  OK(lower_ordered(mps[0], 32, sh, ml, g_bm, &t));
  EQ(t.order, 2, 0, 1);   // by length, descending
  EQ(t.len, 3, 2, 1);
  EQ(t.step_ptr, 0, 3, 5);
  EQ(t.step_code, 4, 3, 4, 0, 1, 2, /* maxL + 8 zero rows */ 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5);
  EQ(t.multi_ptr, 0);
  CHECK(t.multi_rows.empty());
  EQ(t.src_off, 0);
  EQ(t.src_rows, 5);
  CHECK(t.zero_row == 5 && t.n_multi == 0 && t.n_steps == 6 && t.n_msgs == 6 && t.wave_steps == 3);
  CHECK(t.flops == 6 * (2.0 * 32 * 96 + 14 * 32) && t.bytes == 6 * 132.0 + 3 * 256.0 + 16.0);
  CHECK(t.hdr.size() == 64);
  const int want[3][4] = {{2, 3, 0, 4}, {0, 2, 3, 0}, {1, 1, 5, 2}};
  for (int i = 0; i < 16 && t.hdr.size() == 64; ++i)
    for (int k = 0; k < 4; ++k) {
      const int pad[4] = {0, 0, 6, 5};   // {row 0, length 0, n_steps, the zero row}
      CHECK(t.hdr[4 * i + k] == (i < 3 ? want[i][k] : pad[k]));
    }
}
static void ordered_hole_multi_case(int ib) {
  Desc ds = ordered_desc(true);
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_ORDERED, true, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  EQ(ml.mpos, 0, 1, 0, 0, 2, 2);
  EQ(ml.flen, 2, 1, 3);
  OrderedTables t;
  OK(lower_ordered(mps[0], 32, sh, ml, g_bm, &t));
  EQ(t.order, 2, 0, 1);
  EQ(t.step_code, 4, /* hole */ 5, /* multi row 0 */ 6, 0, 1, 2, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5);
  CHECK(t.n_multi == 1 && t.n_msgs == 6);
  EQ(t.multi_ptr, 0, 2);
  EQ(t.multi_rows, 3, 4);   // in message order
  CHECK(t.hdr.size() == 64 && t.hdr[3] == 4);
}

// two sources (entities 0 and 1 -> 2): source 1's slots start after source 0's Lmax of that graph
static void two_source_case(int ib) {
  Desc ds(2, 3, {2, 2, 1, 1, 1, 1},
          {{{{0, 0, 0}, {1, 0, 1}}, {{0, 0, 0}}},    // adjacency 0: Lmax 2, then 1
           {{{1, 0, 0}}, {{0, 0, 0}}}});             // adjacency 1
  std::vector<MPP> mps = {make_mp(2, IGN_AGGR_ORDERED, true, {{0, 0, -1}, {1, 1, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  EQ(ml.mdst, 0, 0, 0, 1, 1);   // per graph: source order, then edge order
  EQ(ml.mpos, 0, 1, 2, 0, 1);
  EQ(ml.mcode, 0, 1, (1 << 29) | 1, 2, (1 << 29) | 2);
  EQ(ml.flen, 3, 2);
  OrderedTables t;
  OK(lower_ordered(mps[0], 32, sh, ml, g_bm, &t));
  EQ(t.src_off, 0, 3);
  EQ(t.src_rows, 3, 3);
  CHECK(t.zero_row == 6);
  EQ(t.order, 0, 1);
  EQ(t.step_ptr, 0, 3);
  EQ(t.step_code, 0, 1, 4, 2, 5, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6);
}

// interleave: A0 B0 A1 B1 on destination 0; destination 1's only message sits at position 2 >= its
// final_len 1 and is dropped (its one step is a hole)
static Desc interleave_desc() {
  Desc ds(1, 3, {2, 2, 2}, {{{{0, 0, 0}, {1, 0, 1}, {0, 1, 1}}}, {{{0, 0, 0}, {1, 0, 1}}}});
  ds.interleave({{{0, 2}}, {{1, 3}}});
  return ds;
}
static void interleave_case(int ib) {
  Desc ds = interleave_desc();
  std::vector<MPP> mps = {make_mp(2, IGN_AGGR_INTERLEAVE, true, {{0, 0, 0}, {1, 1, 1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  EQ(ml.mdst, 0, 0, 1, 0, 0);
  EQ(ml.mpos, 0, 2, 2, 1, 3);
  EQ(ml.flen, 4, 1);
  OrderedTables t;
  OK(lower_ordered(mps[0], 32, sh, ml, g_bm, &t));
  EQ(t.order, 0, 1);
  EQ(t.len, 4, 1);
  EQ(t.src_off, 0, 2);
  EQ(t.step_code, 0, 2, 1, 3, /* the dropped message's destination: a hole */ 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4);
  CHECK(t.n_msgs == 4 && t.n_multi == 0);
}

// ---------------------------------------------------------------------------------------------
// sum MP: entity 0 -> entity 1, G = 2, in-degrees {3, 0, 1} and {2}
static void every_message_once(const MsgLists& ml, const SumCsr& c) {
  std::vector<int> seen(ml.mdst.size(), 0);
  for (size_t i = 0; i + 1 < c.ptr.size(); ++i)
    for (int32_t q = c.ptr[i]; q < c.ptr[i + 1]; ++q) {
      bool found = false;   // message q: an unused message of this destination with this code
      for (size_t k = 0; k < ml.mdst.size() && !found; ++k)
        if (!seen[k] && ml.mdst[k] == c.order[i] && ml.mcode[k] == c.msrc[q]) found = true, seen[k] = 1;
      CHECK(found);
    }
  CHECK(c.ptr.back() == (int32_t)ml.mdst.size());
}
static void sum_case(int ib) {
  Desc ds(2, 2, {2, 3, 2, 1}, {{{{0, 0, 0}, {1, 0, 0}, {1, 2, 0}, {0, 0, 0}}, {{1, 0, 0}, {0, 0, 0}}}});
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_SUM, false, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  EQ(ml.mdst, 0, 0, 2, 0, 3, 3);
  EQ(ml.mcode, 0, 1, 1, 0, 3, 2);
  EQ(ml.flen, 3, 0, 1, 2);
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  EQ(c.order, 0, 3, 2, 1);
  EQ(c.ptr, 0, 3, 5, 6, 6);
  EQ(c.msrc, 0, 1, 0, 3, 2, 1);
  CHECK(c.n_interior == 4 && !c.halo && c.csr_pos.empty());
  every_message_once(ml, c);
  SumAgg ag;
  OK(lower_sum_agg(mps[0], 0, -1, sh, ml, c, &ag));
  CHECK(!ag.window && !ag.seg && ag.n_seg == 0 && ag.id_ptr.empty());
}
// one halo row (source row 2 of 2 owned), G = 1: the destinations that read it come last
static void sum_halo_case(int ib) {
  Desc ds(1, 2, {2, 3}, {{{{0, 0, 0}, {2, 1, 0}, {1, 2, 0}, {1, 1, 0}}}});
  ds.halo = {1, 0};
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_SUM, false, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  EQ(sh.halo, 1, 0);
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  EQ(c.order, 0, 2, 1);
  EQ(c.ptr, 0, 1, 2, 4);
  EQ(c.msrc, 0, 1, 2, 1);
  CHECK(c.n_interior == 2 && c.halo);
  every_message_once(ml, c);
}

// segmented rule: destinations of 64 and 63 messages
static void segmented_case(int ib) {
  std::vector<Edge> e;
  for (int k = 0; k < 64; ++k) e.push_back({k, 0, 0});
  for (int k = 0; k < 63; ++k) e.push_back({k, 1, 0});
  Desc ds(1, 2, {64, 2}, {{e}});
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_SUM, false, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  EQ(c.order, 0, 1);
  EQ(c.ptr, 0, 64, 127);
  {
    SumAgg ag;
    OK(lower_sum_agg(mps[0], 0, -1, sh, ml, c, &ag));
    CHECK(ag.seg && !ag.window && ag.n_seg == 1);
    EQ(ag.id_ptr, 0, 1, 64);
    CHECK(ag.id_src.size() == 64 && ag.id_src[0] == ((1u << IGN_SLOT_SHIFT) | 0u));
    for (size_t k = 1; k < ag.id_src.size(); ++k) CHECK(ag.id_src[k] == k - 1);   // its own 63 codes
  }
  {
    SumAgg ag;
    OK(lower_sum_agg(mps[0], 0, 2, sh, ml, c, &ag));
    CHECK(ag.seg && ag.n_seg == 2);
    EQ(ag.id_ptr, 0, 1, 2);
    EQ(ag.id_src, (1 << 29) | 0, (1 << 29) | 1);
  }
  SumAgg ag;
  FAILS(lower_sum_agg(mps[0], 0, 0, sh, ml, c, &ag), IGN_ERR_UNSUPPORTED, "IGN_SUM_WINDOW=0 (every sum a lane walk): mp 0 has a destination of 64");
}

// windowed tables (sum_window 1): one graph of 257 destinations, 3 source rows
static void windowed_case(int ib) {
  std::vector<Edge> e = {{2, 0, 0}, {1, 0, 0}, {0, 0, 0}};
  for (int dr = 1; dr < 257; ++dr) e.push_back({dr % 3, dr, 0});
  Desc ds(1, 2, {3, 257}, {{e}});
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_SUM, false, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  SumAgg ag;
  OK(lower_sum_agg(mps[0], 0, 1, sh, ml, c, &ag));
  CHECK(ag.window && !ag.seg && ag.n_win_wg == 2);
  EQ(ag.wg, 0, 256, 0, 3, 256, 257, 0, 3);   // {first, last destination slot, the graph's source rows}
  CHECK(ag.wdst.size() == 257 && ag.wptr.size() == 258 && ag.wsrc.size() == 259);
  for (size_t i = 0; i + 1 < ag.wptr.size(); ++i) {
    CHECK(ag.wdst[i] == (int32_t)i);   // by message count, descending, stable: row 0 leads
    CHECK(ag.wptr[i + 1] - ag.wptr[i] == (i == 0 ? 3 : 1));
    for (int32_t q = ag.wptr[i] + 1; q < ag.wptr[i + 1]; ++q) CHECK(ag.wsrc[q - 1] <= ag.wsrc[q]);   // ascending
  }
  CHECK(ag.wsrc[0] == 0 && ag.wsrc[1] == 1 && ag.wsrc[2] == 2);
  CHECK(ag.id_ptr.size() == 258 && ag.id_src.size() == 257);
  for (size_t i = 0; i < ag.id_src.size(); ++i) CHECK(ag.id_ptr[i] == (int32_t)i && ag.id_src[i] == (uint32_t)c.order[i]);
  CHECK(ag.id_ptr.back() == 257);
}

// attention, G = 2: two messages on (destination 0, position 0) share a cell
static void attention_case(int ib) {
  Desc ds(2, 2, {2, 2, 1, 1}, {{{{0, 0, 0}, {1, 0, 0}, {1, 1, 1}}, {{0, 0, 0}}}});
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_ATTENTION, false, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  EQ(ml.mdst, 0, 0, 1, 2);
  EQ(ml.mpos, 0, 0, 1, 0);
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  EQ(c.order, 0, 1, 2);
  EQ(c.ptr, 0, 2, 3, 4);
  EQ(c.csr_pos, 0, 1, 2, 3);
  AttnTables at;
  lower_attention(mps[0], sh, ml, c, &at);
  CHECK(at.n_groups == 3 && at.n_cells == 3);   // groups (graph, position): (0, 0), (0, 1), (1, 0)
  EQ(at.group_ptr, 0, 1, 2, 3);
  EQ(at.group_empty, 1, 1, 0);   // the graph's destinations without a cell in the group
  EQ(at.cell_dst, 0, 1, 2);
  EQ(at.cell_ptr, 0, 2, 3, 4);
  EQ(at.cell_msgs, 0, 1, 2, 3);
}

// ---------------------------------------------------------------------------------------------
// every fail() a small input reaches
static void validation_case(int ib) {
  const std::vector<MPP> ord = {make_mp(1, IGN_AGGR_ORDERED, true, {{0, 0, -1}})};
  const std::vector<MPP> sum = {make_mp(1, IGN_AGGR_SUM, false, {{0, 0, -1}})};
  const std::vector<MPP> att = {make_mp(1, IGN_AGGR_ATTENTION, false, {{0, 0, -1}})};
  const std::vector<MPP> il = {make_mp(2, IGN_AGGR_INTERLEAVE, true, {{0, 0, 0}, {1, 1, 1}})};
  BatchShape sh;
  MsgLists ml;
  auto one = [](std::vector<Edge> e, int64_t nsrc = 2, int64_t ndst = 1) { return Desc(1, 2, {nsrc, ndst}, {{e}}); };
  {
    Desc ds = one({{0, 0, 0}}, -1);
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "graph 0: negative num_ for entity 0");
  }
  {
    Desc ds = one({{0, 0, 0}});
    ds.halo = {1, 0};
    FAILS(lower_to_messages(ds, ib, att, 0, &sh, &ml), IGN_ERR_UNSUPPORTED, "edge-cut partitions support sum and convolution MPs only");
    FAILS(lower_to_messages(ds, ib, ord, 0, &sh, &ml), IGN_ERR_UNSUPPORTED, "edge-cut partitions support sum and convolution MPs only");
    ds.halo = {-1, 0};
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "entity 0: negative halo_rows");
  }
  {
    Desc ds(2, 2, {1, 1, 1, 1}, {{{{0, 0, 0}}, {{0, 0, 0}}}});
    ds.halo = {1, 0};
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "halo rows need num_graphs == 1");
  }
  {
    Desc ds = one({{0, 0, 0}});
    ds.edges[0] = -1;
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "negative edge count");
  }
  {
    Desc ds = one({{0, 0, 0}});
    FAILS(lower_to_messages(ds, 2, sum, 0, &sh, &ml), IGN_ERR_INVALID, "index_bytes 2 (0 / 8: int64 index arrays, 4: int32)");
  }
  {
    Desc ds = interleave_desc();
    ds.interleave({{{0, 2}}, {{1, 3, 0}}});
    FAILS(lower_to_messages(ds, ib, il, 0, &sh, &ml), IGN_ERR_INVALID, "interleave index lists have different lengths (2 vs 3");
    ds.interleave({{{0}}, {{1}}});
    FAILS(lower_to_messages(ds, ib, il, 0, &sh, &ml), IGN_ERR_INVALID, "interleave indices cover 2 slots but the messages need 4");
    ds.interleave({{{0, 2}}, {{1, 4}}});
    FAILS(lower_to_messages(ds, ib, il, 0, &sh, &ml), IGN_ERR_INVALID, "interleave index 4 outside [0,4)");
  }
  {
    Desc ds = one({});
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "graph 0: adjacency slot 0 has no edges");
  }
  {
    Desc ds = one({{0, 0, -1}});
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "graph 0: negative seq value");
  }
  {   // axis-2 concat of sequences of length 2 and 1
    Desc ds(1, 3, {2, 2, 1}, {{{{0, 0, 0}, {1, 0, 1}}}, {{{0, 0, 0}}}});
    std::vector<MPP> cat = {make_mp(2, IGN_AGGR_CONCAT, true, {{0, 0, -1}, {1, 1, -1}})};
    cat[0].feature_concat = true;
    FAILS(lower_to_messages(ds, ib, cat, 0, &sh, &ml), IGN_ERR_INVALID, "concat on axis 2 of sequences of length 2 and 1");
  }
  {
    Desc ds = one({{2, 0, 0}});
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "graph 0: src index 2 out of range [0,2)");
    Desc dn = one({{-1, 0, 0}});
    FAILS(lower_to_messages(dn, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "graph 0: src index -1 out of range [0,2)");
  }
  {
    Desc ds = one({{0, 0, 0}, {1, 1, 0}});
    FAILS(lower_to_messages(ds, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "graph 0: dst index 1 out of range [0,1)");
  }
  {   // two messages on position 0: final_len 2, one padded slot
    Desc ds = one({{0, 0, 0}, {1, 0, 0}});
    FAILS(lower_to_messages(ds, ib, ord, 0, &sh, &ml), IGN_ERR_INVALID, "destination row 0 has final_len 2 > 1 padded slots");
  }
  {   // one message on position 1: the mask is 1 step wide, the padded sequence 2
    Desc ds = one({{0, 0, 1}});
    FAILS(lower_to_messages(ds, ib, ord, 0, &sh, &ml), IGN_ERR_INVALID, "sequence_mask(final_len) is 1 steps wide but the padded sequence has 2");
  }
  {
    Desc ds = one({{0, 0, 0}}, 2, 2);
    OK(lower_to_messages(ds, ib, ord, 0, &sh, &ml));
    OrderedTables t;
    FAILS(lower_ordered(ord[0], 32, sh, ml, g_bm, &t), IGN_ERR_INVALID, "destination row 1 receives no message");
  }
  {   // a message network that reads edge_params, and a desc without them
    Desc ds = one({{0, 0, 0}});
    std::vector<MPP> net = sum;
    net[0].nn[0].inputs = {IGN_MSG_HS_SOURCE, IGN_MSG_EDGE_PARAMS};
    net[0].nn[0].layers.emplace_back();
    OK(lower_to_messages(ds, ib, net, 0, &sh, &ml));
    EQ(ml.mcode, 0);   // the code addresses the edge
    hvec<int32_t> es, ed;
    FAILS(lower_edge_rows(net[0], 0, 0, sh, &es, &ed), IGN_ERR_INVALID, "message network of mp 0 reads edge_params but params_<adj> is missing");
    net[0].nn[0].inputs = {IGN_MSG_HS_SOURCE};
    OK(lower_edge_rows(net[0], 0, 0, sh, &es, &ed));
    EQ(es, 0);
    EQ(ed, 0);
  }
}

// an out-of-range dst index in a graph with zero destination rows, last in the batch; then with no
// row of that entity in the whole batch (the plain fast path used to count it into flen first)
static void empty_destination_case(int ib) {
  const std::vector<MPP> sum = {make_mp(1, IGN_AGGR_SUM, false, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  Desc last(2, 2, {1, 1, 1, 0}, {{{{0, 0, 0}}, {{0, 0, 0}}}});
  FAILS(lower_to_messages(last, ib, sum, 0, &sh, &ml), IGN_ERR_INVALID, "graph 1: dst index 0 out of range [0,0)");
  MsgLists ml2;
  Desc none(1, 2, {1, 0}, {{{{0, 0, 0}}}});
  FAILS(lower_to_messages(none, ib, sum, 0, &sh, &ml2), IGN_ERR_INVALID, "graph 0: dst index 0 out of range [0,0)");
}

// ---------------------------------------------------------------------------------------------
// resident lowering, RouteNet shape: entity 0 = links, 1 = paths; MP 0 ordered links -> paths
// (adjacency 0), MP 1 sum paths -> links (adjacency 1).  Every graph: 3 links, 4 paths
// p0 = l0 l1, p1 = l1 l2, p2 = l2, p3 = l0 l1 l2.
struct Resident {
  BatchShape sh;
  OrderedTables ord;
  SumCsr sum[2];
  ResidentParams rp;
  int lower(Desc& ds, int ib, const std::vector<MPP>& mps, int n_sum) {
    int rc = lower_batch_shape(ds.E, ds.A, ds.IL, mps, ds.make(ib), &sh);
    MsgLists ml;
    if (rc || (rc = lower_messages(mps[0], sh, &ml)) || (rc = lower_ordered(mps[0], 32, sh, ml, g_bm, &ord))) return rc;
    for (int s = 0; s < n_sum; ++s) {
      MsgLists ms;
      if ((rc = lower_messages(mps[1 + s], sh, &ms))) return rc;
      lower_sum_csr(mps[1 + s], sh, ms, g_bm, &sum[s]);
    }
    rp.n_src = n_sum;
    rp.T = 2;
    rp.max_tiles = 32, rp.state_stride = 36, rp.table_stride = 100, rp.max_dyn_lds = 144 * 1024;   // kernels.h
    rp.feature_total.assign(ds.E, 1);
    return IGN_OK;
  }
  void run(int K, ResidentTables* t) {
    const ResOrderedIn ma{ord.order, ord.len, ord.step_ptr, ord.step_code, ord.src_off, ord.zero_row, ord.n_multi, ord.n_steps, ord.flops, ord.bytes};
    std::vector<ResSumIn> sums;
    for (int s = 0; s < rp.n_src; ++s) sums.push_back(ResSumIn{sum[s].order, sum[s].ptr, sum[s].msrc, 0.0, 0.0});
    lower_resident(rp, K, BatchRows{sh.G, sh.row_off, sh.rows, sh.halo}, ma, sums, t);
  }
};
static Desc routenet_desc(int G, bool multi) {
  std::vector<Edge> lp = {{0, 0, 0}, {1, 0, 1}, {1, 1, 0}, {2, 1, 1}, {2, 2, 0}, {0, 3, 0}, {1, 3, 1}, {2, 3, 2}};
  if (multi) lp.push_back({1, 2, 0});   // a second message on p2's position 0
  const std::vector<Edge> pl = {{0, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 2, 0}, {2, 2, 0}, {3, 0, 0}, {3, 1, 0}, {3, 2, 0}};
  std::vector<int64_t> num;
  for (int g = 0; g < G; ++g) num.push_back(3), num.push_back(4);
  return Desc(G, 2, num, {std::vector<std::vector<Edge>>(G, lp), std::vector<std::vector<Edge>>(G, pl)});
}
static const std::vector<MPP>& routenet_mps() {
  static const std::vector<MPP> mps = {make_mp(1, IGN_AGGR_ORDERED, true, {{0, 0, -1}}), make_mp(0, IGN_AGGR_SUM, false, {{1, 1, -1}})};
  return mps;
}
static void expect_hdr(const ResidentTables& t, size_t first, std::initializer_list<std::initializer_list<int>> rows,
                       std::initializer_list<int> pad, std::initializer_list<int> hsb, int hsb_pad, int line) {
  std::vector<int> want, wh(hsb);
  for (auto& r : rows) want.insert(want.end(), r.begin(), r.end());
  while (want.size() < 64) want.insert(want.end(), pad.begin(), pad.end());   // padded to a whole tile
  wh.resize(16, hsb_pad);
  bool ok = t.hdr.size() >= 4 * first + 64 && t.hsb.size() >= first + 16;
  for (size_t i = 0; ok && i < 64; ++i) ok = t.hdr[4 * first + i] == want[i];
  for (size_t i = 0; ok && i < 16; ++i) ok = t.hsb[first + i] == wh[i];
  if (!ok) printf("FAIL [%s] line %d: hdr / hsb of the tile at %zu\n", g_case, line, first), ++g_bad;
}
static void resident_case(int ib) {
  Desc ds = routenet_desc(2, false);
  Resident r;
  r.rp.path = 1, r.rp.src_ent[0] = 0;
  OK(r.lower(ds, ib, routenet_mps(), 1));
  EQ(r.ord.order, 3, 7, 0, 1, 4, 5, 2, 6);
  EQ(r.ord.step_ptr, 0, 3, 6, 8, 10, 12, 14, 15);
  EQ(r.sum[0].order, 1, 2, 4, 5, 0, 3);
  EQ(r.sum[0].msrc, 0, 1, 3, 1, 2, 3, 4, 5, 7, 5, 6, 7, 0, 3, 4, 7);
  {
    ResidentTables t;
    r.run(1, &t);
    CHECK(t.eligible && t.K == 1 && t.G == 2 && t.form == kResAllLds && t.train_form == kResPathGlobal);
    EQ(t.path_off, 0, 4, 8);
    EQ(t.src_off[0], 0, 3, 6);
    EQ(t.urow_off, 0, 3, 6);
    EQ(t.lmsg_ptr, 0, 2, 5, 8, 0, 2, 5, 8);
    EQ(t.lmsg_off, 0, 8, 16);
    EQ(t.lmsg_src, 0, 3, 0, 1, 3, 1, 2, 3, 0, 3, 0, 1, 3, 1, 2, 3);
    EQ(t.lorder, 1, 2, 0, 1, 2, 0);
    EQ(t.lnseg, 0, 0);
    EQ(t.gorder, 0, 1);
    EQ(t.ptile_off, 0, 16, 32);
    EQ(t.lcode_off, 0, 19, 38);
    EQ(t.lcode, 0, 1, 2, 0, 1, 1, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3,   // 8 codes, then 3 + 8 holes (U = 3)
       0, 1, 2, 0, 1, 1, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3);
    // {local path row, length, local step offset, first code}; padding {-1, 0, the graph's codes, the hole}
    expect_hdr(t, 0, {{3, 3, 0, 0}, {0, 2, 3, 0}, {1, 2, 5, 1}, {2, 1, 7, 2}}, {-1, 0, 8, 3}, {0, 8, 11, 20}, 24, __LINE__);
    expect_hdr(t, 16, {{3, 3, 0, 0}, {0, 2, 3, 0}, {1, 2, 5, 1}, {2, 1, 7, 2}}, {-1, 0, 8, 3}, {4, 14, 17, 22}, 24, __LINE__);
    CHECK(t.lds[0] == 2686 && t.lds[1] == 2072 && t.lds[2] == 2056);
    CHECK(t.info.active == 1 && t.info.workgroups == 2 && t.info.graphs_per_workgroup == 1 && t.info.lds_bytes == 2686);
    CHECK(t.info.messages == 16 && t.info.seg_rows == 0 && t.info.union_tiles == 2 && t.info.tile_steps == 2 * 6);
  }
  {
    ResidentTables t;
    r.run(2, &t);
    CHECK(t.eligible && t.K == 2 && t.G == 1 && t.form == kResAllLds);
    EQ(t.path_off, 0, 8);
    EQ(t.src_off[0], 0, 6);
    EQ(t.urow_off, 0, 6);
    EQ(t.lmsg_ptr, 0, 2, 5, 8, 10, 13, 16);
    EQ(t.lmsg_off, 0, 16);
    EQ(t.lmsg_src, 0, 3, 0, 1, 3, 1, 2, 3, 4, 7, 4, 5, 7, 5, 6, 7);
    EQ(t.lorder, 1, 2, 4, 5, 0, 3);
    EQ(t.lnseg, 0);
    EQ(t.gorder, 0);
    EQ(t.ptile_off, 0, 16);
    EQ(t.lcode_off, 0, 27);
    EQ(t.lcode, 0, 1, 2, 3, 4, 5, 0, 1, 1, 2, 3, 4, 4, 5, 2, 5, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6);
    expect_hdr(t, 0, {{3, 3, 0, 0}, {7, 3, 3, 3}, {0, 2, 6, 0}, {1, 2, 8, 1}, {4, 2, 10, 3}, {5, 2, 12, 4}, {2, 1, 14, 2}, {6, 1, 15, 5}},
               {-1, 0, 16, 6}, {0, 4, 8, 11, 14, 17, 20, 22}, 24, __LINE__);
    CHECK(t.lds[0] == 4942 && t.lds[1] == 3736 && t.lds[2] == 3704);
    CHECK(t.info.workgroups == 1 && t.info.graphs_per_workgroup == 2 && t.info.tile_steps == 2 * 3);
  }
  {   // three graphs, two per workgroup: the last group holds one
    Desc d3 = routenet_desc(3, false);
    Resident r3;
    r3.rp.path = 1, r3.rp.src_ent[0] = 0;
    OK(r3.lower(d3, ib, routenet_mps(), 1));
    ResidentTables t;
    r3.run(2, &t);
    CHECK(t.eligible && t.G == 2 && t.info.workgroups == 2);
    EQ(t.path_off, 0, 8, 12);
    EQ(t.src_off[0], 0, 6, 9);
    EQ(t.urow_off, 0, 6, 9);
    EQ(t.ptile_off, 0, 16, 32);
    EQ(t.lcode_off, 0, 27, 46);
    EQ(t.lmsg_off, 0, 16, 24);
    EQ(t.gorder, 0, 1);
    expect_hdr(t, 16, {{3, 3, 0, 0}, {0, 2, 3, 0}, {1, 2, 5, 1}, {2, 1, 7, 2}}, {-1, 0, 8, 3}, {6 + 2, 17 + 7, 19 + 8, 23 + 11}, 36, __LINE__);   // step_ptr + position
  }
  {   // a multi row in the ordered MP: not eligible
    Desc dm = routenet_desc(2, true);
    Resident rm;
    rm.rp.path = 1, rm.rp.src_ent[0] = 0;
    OK(rm.lower(dm, ib, routenet_mps(), 1));
    CHECK(rm.ord.n_multi == 2);
    ResidentTables t;
    rm.run(1, &t);
    CHECK(!t.eligible);
  }
}
// The byte budget's edges on the fixture above (per graph 2686 / 2072 / 2056 bytes in the all-LDS, path-global
// and CSR-global forms; 4942 / 3736 / 3704 for two graphs in one workgroup), with max_dyn_lds moved onto and
// one byte under each: the form, the training form (path states always global) and whether the batch lowers.
// (The 16-bit row limit has no tiny instance: tests/test_gpu_resident_cases.py holds it at 65 535 paths.)
static void resident_budget_case(int ib) {
  Desc ds = routenet_desc(2, false);
  Resident r;
  r.rp.path = 1, r.rp.src_ent[0] = 0;
  OK(r.lower(ds, ib, routenet_mps(), 1));
  const struct { size_t max; bool pg_ok, force; int K; bool eligible; int form, train_form; } rows[] = {
      // A: all-LDS <-> path-global
      {2686, true, false, 1, true, kResAllLds, kResPathGlobal},
      {2685, true, false, 1, true, kResPathGlobal, kResPathGlobal},
      {2686, false, false, 1, true, kResAllLds, kResPathGlobal},
      {2685, false, false, 1, false, 0, 0},                          // IGN_RESIDENT_PG=0: no other form
      {2686, true, true, 1, true, kResPathGlobal, kResPathGlobal},   // IGN_RESIDENT=2
      // B: path-global <-> CSR-global (the training form moves with it)
      {2072, true, false, 1, true, kResPathGlobal, kResPathGlobal},
      {2071, true, false, 1, true, kResPathCsrGlobal, kResPathCsrGlobal},
      {2071, true, true, 1, true, kResPathCsrGlobal, kResPathCsrGlobal},
      // C: CSR-global <-> not resident
      {2056, true, false, 1, true, kResPathCsrGlobal, kResPathCsrGlobal},
      {2055, true, false, 1, false, 0, 0},
      // D: two graphs per workgroup: the union's own bytes decide its form, and whether it lowers at all
      {4942, true, false, 2, true, kResAllLds, kResPathGlobal},
      {4941, true, false, 2, true, kResPathGlobal, kResPathGlobal},
      {3736, true, false, 2, true, kResPathGlobal, kResPathGlobal},
      {3735, true, false, 2, true, kResPathCsrGlobal, kResPathCsrGlobal},
      {3704, true, false, 2, true, kResPathCsrGlobal, kResPathCsrGlobal},
      {3703, true, false, 2, false, 0, 0}};                          // (one graph per workgroup still lowers: 2056)
  for (const auto& w : rows) {
    r.rp.max_dyn_lds = w.max, r.rp.path_global_ok = w.pg_ok, r.rp.force_path_global = w.force;
    ResidentTables t;
    r.run(w.K, &t);
    bool ok = t.eligible == w.eligible;
    if (ok && w.eligible) {
      static const size_t one[3] = {2686, 2072, 2056}, two[3] = {4942, 3736, 3704};
      const size_t* want = w.K == 1 ? one : two;
      ok = t.form == w.form && t.train_form == w.train_form && t.K == w.K && t.G == (w.K == 1 ? 2 : 1) &&
           t.lds[0] == want[0] && t.lds[1] == want[1] && t.lds[2] == want[2] && t.info.lds_bytes == (int64_t)want[w.form] &&
           t.info.form == w.form && t.info.graphs_per_workgroup == w.K && t.info.workgroups == t.G;
    }
    if (!ok) printf("FAIL [%s]: max_dyn_lds %zu, K %d, pg_ok %d, force %d\n", g_case, w.max, w.K, w.pg_ok, w.force), ++g_bad;
  }
  // the automatic rule of the engine (two graphs per workgroup where one graph's all-LDS bytes fit twice)
  // never asks for a union that needs another form: the union's bytes are at most twice one graph's
  CHECK(4942 <= 2 * 2686 && 3736 <= 2 * 2072 && 3704 <= 2 * 2056);
  // the tile limit: a graph's 3 links are one union-row tile
  r.rp.max_dyn_lds = 144 * 1024, r.rp.path_global_ok = true, r.rp.force_path_global = false;
  for (int tiles : {1, 0}) {
    r.rp.max_tiles = tiles;
    ResidentTables t;
    r.run(2, &t);
    CHECK(t.eligible == (tiles == 1));
  }
}
// Q-size shape, one small graph: entities 0 = links, 1 = nodes, 2 = paths; the path is l0 n0 l1 n1.
// Union rows: entity 0's rows, then entity 1's
static void resident_two_source_case(int ib) {
  Desc ds(1, 3, {2, 2, 1},
          {{{{0, 0, 0}, {1, 0, 1}}}, {{{0, 0, 0}, {1, 0, 1}}}, {{{0, 0, 0}, {0, 1, 0}}}, {{{0, 0, 0}, {0, 1, 0}}}});
  ds.interleave({{{0, 2}}, {{1, 3}}});
  const std::vector<MPP> mps = {make_mp(2, IGN_AGGR_INTERLEAVE, true, {{0, 0, 0}, {1, 1, 1}}),
                                make_mp(0, IGN_AGGR_SUM, false, {{2, 2, -1}}), make_mp(1, IGN_AGGR_SUM, false, {{2, 3, -1}})};
  Resident r;
  r.rp.path = 2, r.rp.src_ent[0] = 0, r.rp.src_ent[1] = 1;
  OK(r.lower(ds, ib, mps, 2));
  EQ(r.ord.src_off, 0, 2);
  EQ(r.ord.step_code, 0, 2, 1, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4);
  ResidentTables t;
  r.run(1, &t);
  CHECK(t.eligible && t.G == 1);
  EQ(t.src_off[0], 0, 2);
  EQ(t.src_off[1], 0, 2);
  EQ(t.urow_off, 0, 4);
  EQ(t.lcode, 0, 2, 1, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4);   // links 0..1, nodes 2..3, the hole 4
  EQ(t.lmsg_ptr, 0, 1, 2, 3, 4);
  EQ(t.lmsg_src, 0, 0, 0, 0);
  EQ(t.lorder, 0, 1, 2, 3);
  expect_hdr(t, 0, {{0, 4, 0, 0}}, {-1, 0, 4, 4}, {0}, 5, __LINE__);
  CHECK(t.info.union_tiles == 2);
}

int main() {
  const struct { const char* name; void (*fn)(int); } cases[] = {
      {"ordered", ordered_case}, {"ordered hole+multi", ordered_hole_multi_case}, {"two sources", two_source_case},
      {"interleave", interleave_case}, {"sum", sum_case}, {"sum halo", sum_halo_case}, {"segmented", segmented_case},
      {"windowed", windowed_case}, {"attention", attention_case}, {"validation", validation_case},
      {"empty destination", empty_destination_case}, {"resident", resident_case},
      {"resident budget", resident_budget_case}, {"resident two sources", resident_two_source_case}};
  // every case at both index widths against the same hand tables: int32 and int64 descs lower equally
  for (int ib : {8, 4})
    for (auto& c : cases) {
      char name[96];
      snprintf(name, sizeof name, "%s, index_bytes %d", c.name, ib);
      g_case = name;
      const int before = g_bad;
      c.fn(ib);
      printf("%s [%s]\n", g_bad == before ? "ok  " : "FAIL", name);
    }
  printf("%d failed checks\n", g_bad);
  return g_bad ? 1 : 0;
}
