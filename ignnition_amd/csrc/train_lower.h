// train_lower.h — the host-side lowering of a batch's training tables: the transposed CSRs the
// backward walks, from the host copies of the index tables the batch keeps.  Pure host code (no HIP
// header, no device or pool call), so it runs and is checked on a CPU (tests/cpp/train_lower_check.cpp);
// train_alloc.cpp uploads what it returns.  The source row -> steps / destinations tables also have a GPU
// builder (train_csr.hip, the default where no pre-summed row is involved); the others are built here only.
#pragma once
#include <utility>

#include "host_types.h"

namespace ign {

// CSR of (key, value) pairs over n_keys keys, values kept in insertion order per key
void build_csr(int64_t n_keys, const hvec<std::pair<int64_t, int32_t>>& kv, hvec<int32_t>& ptr, hvec<int32_t>& idx);

// Per source slot s, the CSR of the (row, value) pairs visit() emits, values in emission order
// per row: one counting pass and one filling pass over the same visit, no pair list.
template <class Visit>
void build_csrs(int S, const int64_t* n_keys, Visit visit, std::vector<hvec<int32_t>>& ptr,
                std::vector<hvec<int32_t>>& idx) {
  ptr.assign(S, hvec<int32_t>());
  idx.assign(S, hvec<int32_t>());
  for (int s = 0; s < S; ++s) ptr[s].assign(n_keys[s] + 1, 0);
  visit([&](int s, int64_t key, int32_t) { ptr[s][key + 1]++; });
  std::vector<hvec<int32_t>> fill(S);
  for (int s = 0; s < S; ++s) {
    for (int64_t k = 0; k < n_keys[s]; ++k) ptr[s][k + 1] += ptr[s][k];
    idx[s].resize(ptr[s][n_keys[s]]);
    fill[s].assign(ptr[s].begin(), ptr[s].end() - 1);
  }
  visit([&](int s, int64_t key, int32_t v) { idx[s][fill[s][key]++] = v; });
}

// the host tables of one MP (the batch's MPB host copies): ordered MPs read order .. multi_rows,
// src_off and zero_row; sum MPs h_order, h_msg_ptr and h_msg_src
struct TrainMpIn {
  const hvec<int32_t>&h_order, &h_len, &h_step_ptr, &h_msg_ptr, &h_multi_ptr;
  const hvec<uint32_t>&h_step_code, &h_msg_src, &h_multi_rows;
  const std::vector<int64_t>& src_off;
  int64_t zero_row, n_dst, n_msgs;
};

// keys of source slot s's tables: its entity's rows plus halo, or its edges under a message network
inline int64_t train_keys(const MPP& mp, int s, const std::vector<int64_t>& rows, const std::vector<int64_t>& halo,
                          const int64_t* n_edges) {
  return mp.nn[s].layers.empty() ? rows[mp.src[s].entity] + halo[mp.src[s].entity] : n_edges[s];
}

// ordered MP, per source slot: source row -> steps whose input contains it (directly or through a
// pre-summed row)
void lower_train_ordered(int S, const int64_t* keys, const TrainMpIn& mb, std::vector<hvec<int32_t>>& ptr,
                         std::vector<hvec<int32_t>>& idx);

// sum MP, per source slot: source row -> destination rows reading it, in h_order order
void lower_train_sum(int S, const int64_t* keys, const TrainMpIn& mb, std::vector<hvec<int32_t>>& ptr,
                     std::vector<hvec<int32_t>>& idx);

// attention (AUX:287-343): message -> destination row, and per source slot row -> messages
struct TrainAttn {
  hvec<int32_t> mdst;
  std::vector<hvec<int32_t>> ptr, idx;
};
void lower_train_attention(int S, const int64_t* keys, const TrainMpIn& mb, TrainAttn* out);

// convolution: messages per destination row
void lower_train_degree(const TrainMpIn& mb, hvec<float>* deg);

// row -> the edges e with row_of_edge[e] == row, ascending: a message network's source state row /
// destination row -> edges (GM:440-475), an extend_adjacencies op's input row -> edges
void lower_row_edges(int64_t n_rows, const int32_t* row_of_edge, int64_t n_edges, hvec<int32_t>* ptr, hvec<int32_t>* idx);

}  // namespace ign
