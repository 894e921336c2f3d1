// train_lower_check.cpp — stand-alone check of ignnition_amd/csrc/train_lower.cpp (no GPU, no HIP):
// the smallest cases in which each builder of the training tables can still go wrong, every expected
// table written out by hand.  Where the batch lowering (batch_lower.cpp) accepts the case, it produces
// the host tables the builders read; a graph without destination rows and an MP without messages it
// refuses, so those tables are typed in.  tests/test_train_lower.py builds this with g++, plain and
// under -fsanitize=address,undefined, and runs it; a non-zero exit is a failure.
#include "lower_check.h"

#include "../../ignnition_amd/csrc/train_lower.h"

// one MP's host tables, as the batch keeps them (MPB's h_* copies)
struct Host {
  hvec<int32_t> order, len, step_ptr, msg_ptr, multi_ptr;
  hvec<uint32_t> step_code, msg_src, multi_rows;
  std::vector<int64_t> src_off;
  int64_t zero_row = 0, n_dst = 0, n_msgs = 0;
  TrainMpIn in() const {
    return {order, len, step_ptr, msg_ptr, multi_ptr, step_code, msg_src, multi_rows, src_off, zero_row, n_dst, n_msgs};
  }
};
static Host host_of(const OrderedTables& t) {
  Host h;
  h.order = t.order, h.len = t.len, h.step_ptr = t.step_ptr, h.multi_ptr = t.multi_ptr;
  h.step_code = t.step_code, h.multi_rows = t.multi_rows;
  h.src_off = t.src_off, h.zero_row = t.zero_row, h.n_dst = (int64_t)t.order.size(), h.n_msgs = t.n_msgs;
  return h;
}
static Host host_of(const SumCsr& c) {
  Host h;
  h.order = c.order, h.msg_ptr = c.ptr, h.msg_src = c.msrc;
  h.n_dst = (int64_t)c.order.size(), h.n_msgs = (int64_t)c.msrc.size();
  return h;
}

// what every CSR satisfies: ptr over keys + 1 entries from 0 to idx.size(), non-decreasing, and each
// row's values in emission order (rank[v]: when value v is emitted; empty: ascending values)
#define CSR_OK(ptr, idx, keys, ...) csr_ok(#ptr, __LINE__, ptr, idx, keys, {__VA_ARGS__})
static void csr_ok(const char* what, int line, const hvec<int32_t>& ptr, const hvec<int32_t>& idx, int64_t keys,
                   std::vector<int> rank) {
  bool ok = (int64_t)ptr.size() == keys + 1 && ptr[0] == 0 && ptr.back() == (int32_t)idx.size();
  for (size_t k = 0; ok && k + 1 < ptr.size(); ++k) {
    ok = ptr[k] <= ptr[k + 1];
    for (int32_t q = ptr[k] + 1; ok && q < ptr[k + 1]; ++q)
      ok = rank.empty() ? idx[q - 1] <= idx[q] : rank[idx[q - 1]] <= rank[idx[q]];
  }
  if (!ok) printf("FAIL [%s] line %d: %s is no CSR in emission order\n", g_case, line, what), ++g_bad;
}

// ordered, one source (links -> paths): links l0 and l1 on position 0 of path 0 (one pre-summed table
// row), a hole at position 1, l2 at position 2; path 1 reads l2
static void ordered_multi_case(int ib) {
  Desc ds(1, 2, {3, 2}, {{{{0, 0, 0}, {1, 0, 0}, {2, 0, 2}, {2, 1, 0}}}});
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_ORDERED, true, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  OrderedTables t;
  OK(lower_ordered(mps[0], 32, sh, ml, g_bm, &t));
  CHECK(t.n_multi == 1 && t.zero_row == 3 && t.n_steps == 4);
  EQ(t.order, 0, 1);
  EQ(t.len, 3, 1);
  EQ(t.step_ptr, 0, 3);
  CHECK(t.step_code.size() >= 4 && t.step_code[0] == 4 /* multi row 0 */ && t.step_code[1] == 3 /* hole */ &&
        t.step_code[2] == 2 && t.step_code[3] == 2);
  EQ(t.multi_ptr, 0, 2);
  EQ(t.multi_rows, 0, 1);
  const Host h = host_of(t);
  const int64_t keys[1] = {train_keys(mps[0], 0, sh.rows, sh.halo, nullptr)};
  CHECK(keys[0] == 3);
  std::vector<hvec<int32_t>> ptr, idx;
  lower_train_ordered(1, keys, h.in(), ptr, idx);
  CHECK(ptr.size() == 1 && idx.size() == 1);
  EQ(ptr[0], 0, 1, 2, 4);
  EQ(idx[0], 0, 0, 2, 3);   // step 0 under both summed rows
  CSR_OK(ptr[0], idx[0], 3);
}

// ordered, two sources (links, nodes -> paths; test_oracle.holes_input's adjacencies): the nodes'
// slots start after the links' Lmax 2.  p0 = l0 l1 n0, p1 = l1 - n1 (n2 on position 3 >= final_len 3
// is dropped), p2 = l0 l1 n1 n2.  Table rows: links 0..1, nodes 2..4, the zero row 5
static void ordered_two_source_case(int ib) {
  Desc ds(1, 3, {2, 3, 3},
          {{{{0, 0, 0}, {1, 0, 1}, {1, 1, 0}, {0, 2, 0}, {1, 2, 1}}}, {{{0, 0, 0}, {1, 1, 0}, {2, 1, 1}, {1, 2, 0}, {2, 2, 1}}}});
  std::vector<MPP> mps = {make_mp(2, IGN_AGGR_ORDERED, true, {{0, 0, -1}, {1, 1, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  OrderedTables t;
  OK(lower_ordered(mps[0], 32, sh, ml, g_bm, &t));
  EQ(t.src_off, 0, 2);
  CHECK(t.zero_row == 5 && t.n_multi == 0 && t.n_steps == 10);
  EQ(t.order, 2, 0, 1);
  EQ(t.step_ptr, 0, 4, 7);
  CHECK(t.step_code.size() >= 10);
  const uint32_t codes[10] = {0, 1, 3, 4, /* p0 */ 0, 1, 2, /* p1 */ 1, 5, 3};
  for (int i = 0; i < 10 && t.step_code.size() >= 10; ++i) CHECK(t.step_code[i] == codes[i]);
  const Host h = host_of(t);
  const int64_t keys[2] = {train_keys(mps[0], 0, sh.rows, sh.halo, nullptr), train_keys(mps[0], 1, sh.rows, sh.halo, nullptr)};
  CHECK(keys[0] == 2 && keys[1] == 3);
  std::vector<hvec<int32_t>> ptr, idx;
  lower_train_ordered(2, keys, h.in(), ptr, idx);
  CHECK(ptr.size() == 2 && idx.size() == 2);
  EQ(ptr[0], 0, 2, 5);
  EQ(idx[0], 0, 4, 1, 5, 7);
  EQ(ptr[1], 0, 1, 3, 4);      // n0 is table row 2 = src_off[1]: row 0 of slot 1, not row 2 of slot 0
  EQ(idx[1], 6, 2, 9, 3);
  CSR_OK(ptr[0], idx[0], 2);
  CSR_OK(ptr[1], idx[1], 3);
}

// sum, two source slots A and B, G = 2: graph 0 has rows A0 A1, B0 B1 and destinations d0 <- A0 A1 B1,
// d1 <- A1, d2 <- A1 B1; graph 1, last in the batch, has A2 and B2 and no destination row
static void sum_two_slot_case(int) {
  const uint32_t B = 1u << IGN_SLOT_SHIFT;
  Host h;
  h.order = {0, 2, 1};   // by message count
  h.msg_ptr = {0, 3, 5, 6};
  h.msg_src = {0, 1, B | 1, 1, B | 1, 1};
  h.n_dst = 3, h.n_msgs = 6;
  const int64_t keys[2] = {3, 3};
  std::vector<hvec<int32_t>> ptr, idx;
  lower_train_sum(2, keys, h.in(), ptr, idx);
  CHECK(ptr.size() == 2 && idx.size() == 2);
  EQ(ptr[0], 0, 1, 4, 4);   // A2: the last graph's row, read by nothing
  EQ(idx[0], 0, 0, 2, 1);   // A1's readers in h_order order, not ascending
  EQ(ptr[1], 0, 0, 2, 2);   // B0 without a message
  EQ(idx[1], 0, 2);
  CSR_OK(ptr[0], idx[0], 3, 0, 2, 1);   // rank of destination rows 0, 1, 2 in h_order
  CSR_OK(ptr[1], idx[1], 3, 0, 2, 1);
}

// attention with two sources A, B -> d: d0 <- A1 B0, d1 <- A0 A1 B1
static void attention_two_source_case(int ib) {
  Desc ds(1, 3, {2, 2, 2}, {{{{0, 1, 0}, {1, 1, 1}, {1, 0, 0}}}, {{{0, 0, 0}, {1, 1, 0}}}});
  std::vector<MPP> mps = {make_mp(2, IGN_AGGR_ATTENTION, false, {{0, 0, -1}, {1, 1, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  const int B = 1 << IGN_SLOT_SHIFT;
  EQ(c.order, 1, 0);
  EQ(c.ptr, 0, 3, 5);
  EQ(c.msrc, 0, 1, B | 1, 1, B | 0);
  const Host h = host_of(c);
  const int64_t keys[2] = {train_keys(mps[0], 0, sh.rows, sh.halo, nullptr), train_keys(mps[0], 1, sh.rows, sh.halo, nullptr)};
  CHECK(keys[0] == 2 && keys[1] == 2);
  TrainAttn at;
  lower_train_attention(2, keys, h.in(), &at);
  EQ(at.mdst, 1, 1, 1, 0, 0);
  CHECK(at.ptr.size() == 2 && at.idx.size() == 2);
  EQ(at.ptr[0], 0, 1, 3);
  EQ(at.idx[0], 0, 1, 3);
  EQ(at.ptr[1], 0, 1, 2);
  EQ(at.idx[1], 4, 2);
  CSR_OK(at.ptr[0], at.idx[0], 2);
  CSR_OK(at.ptr[1], at.idx[1], 2);
}

// convolution, G = 2, in-degrees {3, 0, 1} and {2}
static void convolution_case(int ib) {
  Desc ds(2, 2, {2, 3, 2, 1}, {{{{0, 0, 0}, {1, 0, 0}, {1, 2, 0}, {0, 0, 0}}, {{1, 0, 0}, {0, 0, 0}}}});
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_CONVOLUTION, false, {{0, 0, -1}})};
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  EQ(c.order, 0, 3, 2, 1);
  EQ(c.ptr, 0, 3, 5, 6, 6);
  hvec<float> deg;
  lower_train_degree(host_of(c).in(), &deg);
  EQ(deg, 3, 0, 1, 2);   // by destination row
}

// message network on a sum MP: 2 owned source rows and one halo row, 4 destination rows; edges
// 0 -> d0, 2 (halo) -> d1, 1 -> d2, 1 -> d1; d3 has no edge
static void message_network_case(int ib) {
  Desc ds(1, 2, {2, 4}, {{{{0, 0, 0}, {2, 1, 0}, {1, 2, 0}, {1, 1, 0}}}});
  ds.halo = {1, 0};
  std::vector<MPP> mps = {make_mp(1, IGN_AGGR_SUM, false, {{0, 0, -1}})};
  mps[0].nn[0].inputs = {IGN_MSG_HS_SOURCE, IGN_MSG_HS_DEST};
  mps[0].nn[0].layers.emplace_back();
  BatchShape sh;
  MsgLists ml;
  OK(lower_to_messages(ds, ib, mps, 0, &sh, &ml));
  hvec<int32_t> es, ed;
  OK(lower_edge_rows(mps[0], 0, 0, sh, &es, &ed));
  EQ(es, 0, 2, 1, 1);
  EQ(ed, 0, 1, 2, 1);
  hvec<int32_t> p1, i1, p2, i2;
  lower_row_edges(sh.rows[0] + sh.halo[0], es.data(), 4, &p1, &i1);
  lower_row_edges(sh.rows[1], ed.data(), 4, &p2, &i2);
  EQ(p1, 0, 1, 3, 4);   // keys run to rows + halo
  EQ(i1, 0, 2, 3, 1);
  EQ(p2, 0, 1, 3, 4, 4);
  EQ(i2, 0, 1, 3, 2);
  CSR_OK(p1, i1, 3);
  CSR_OK(p2, i2, 4);
  // the MP's own table: the codes address the edges, so its keys are the edges
  const int64_t n_edges[IGN_MAX_SLOTS] = {4, 0, 0, 0};
  const int64_t keys[1] = {train_keys(mps[0], 0, sh.rows, sh.halo, n_edges)};
  CHECK(keys[0] == 4);
  SumCsr c;
  lower_sum_csr(mps[0], sh, ml, g_bm, &c);
  EQ(c.order, 1, 0, 2, 3);
  EQ(c.msrc, 1, 3, 0, 2);
  std::vector<hvec<int32_t>> ptr, idx;
  lower_train_sum(1, keys, host_of(c).in(), ptr, idx);
  CHECK(ptr.size() == 1 && idx.size() == 1);
  EQ(ptr[0], 0, 1, 2, 3, 4);
  EQ(idx[0], 0, 1, 2, 1);
}

// extend_adjacencies: input 0 on a space of 4 rows (rows 1 and 3 read by no edge), input 1 on 2 rows
static void extend_case(int) {
  const std::vector<int32_t> ix0 = {0, 2, 2}, ix1 = {1, 0, 1};
  hvec<int32_t> p0, i0, p1, i1;
  lower_row_edges(4, ix0.data(), (int64_t)ix0.size(), &p0, &i0);
  lower_row_edges(2, ix1.data(), (int64_t)ix1.size(), &p1, &i1);
  EQ(p0, 0, 1, 1, 3, 3);
  EQ(i0, 0, 1, 2);
  EQ(p1, 0, 1, 3);
  EQ(i1, 1, 0, 2);
  CSR_OK(p0, i0, 4);
  CSR_OK(p1, i1, 2);
}

// no message at all, over two destination rows and slots of 3 and 2 keys: every ptr keys + 1 zeros,
// every idx empty; the empty tables' data() may be null
static void empty_case(int) {
  const int64_t keys[2] = {3, 2};
  auto all_empty = [&](const std::vector<hvec<int32_t>>& ptr, const std::vector<hvec<int32_t>>& idx) {
    CHECK(ptr.size() == 2 && idx.size() == 2);
    if (ptr.size() != 2 || idx.size() != 2) return;
    EQ(ptr[0], 0, 0, 0, 0);
    EQ(ptr[1], 0, 0, 0);
    CHECK(idx[0].empty() && idx[1].empty());
    CSR_OK(ptr[0], idx[0], 3);
    CSR_OK(ptr[1], idx[1], 2);
  };
  Host sum;
  sum.order = {0, 1};
  sum.msg_ptr = {0, 0, 0};
  sum.n_dst = 2;
  std::vector<hvec<int32_t>> ptr, idx;
  lower_train_sum(2, keys, sum.in(), ptr, idx);
  all_empty(ptr, idx);
  TrainAttn at;
  lower_train_attention(2, keys, sum.in(), &at);
  CHECK(at.mdst.empty());
  all_empty(at.ptr, at.idx);
  hvec<float> deg;
  lower_train_degree(sum.in(), &deg);
  EQ(deg, 0, 0);
  Host ord;   // two destinations of length 0
  ord.order = {0, 1};
  ord.len = {0, 0};
  ord.step_ptr = {0, 0};
  ord.multi_ptr = {0};
  ord.src_off = {0, 3};
  ord.zero_row = 5, ord.n_dst = 2;
  lower_train_ordered(2, keys, ord.in(), ptr, idx);
  all_empty(ptr, idx);
  Host none;   // no destination row either
  none.msg_ptr = {0};
  lower_train_sum(2, keys, none.in(), ptr, idx);
  all_empty(ptr, idx);
  lower_train_degree(none.in(), &deg);
  CHECK(deg.empty());
  const hvec<int32_t> no_edges;
  hvec<int32_t> p, i;
  lower_row_edges(3, no_edges.data(), 0, &p, &i);
  EQ(p, 0, 0, 0, 0);
  CHECK(i.empty());
  CSR_OK(p, i, 3);
}

int main() {
  const struct { const char* name; void (*fn)(int); } cases[] = {
      {"ordered multi", ordered_multi_case}, {"ordered two sources", ordered_two_source_case},
      {"sum two slots", sum_two_slot_case}, {"attention two sources", attention_two_source_case},
      {"convolution", convolution_case}, {"message network", message_network_case}, {"extend", extend_case},
      {"empty", empty_case}};
  // every case at both index widths of the desc (the typed-in tables have none)
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
