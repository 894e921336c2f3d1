// train_lower.cpp — see train_lower.h
#include "train_lower.h"

namespace ign {

void build_csr(int64_t n_keys, const hvec<std::pair<int64_t, int32_t>>& kv, hvec<int32_t>& ptr,
               hvec<int32_t>& idx) {
  ptr.assign(n_keys + 1, 0);
  for (auto& p : kv) ptr[p.first + 1]++;
  for (int64_t k = 0; k < n_keys; ++k) ptr[k + 1] += ptr[k];
  idx.resize(kv.size());
  hvec<int32_t> fill(ptr.begin(), ptr.end() - 1);
  for (auto& p : kv) idx[fill[p.first]++] = p.second;
}

void lower_train_ordered(int S, const int64_t* keys, const TrainMpIn& mb, std::vector<hvec<int32_t>>& ptr,
                         std::vector<hvec<int32_t>>& idx) {
  build_csrs(S, keys, [&](auto&& emit) {
    auto add_row = [&](uint32_t trow, int32_t step) {
      for (int s = S - 1; s >= 0; --s)
        if ((int64_t)trow >= mb.src_off[s]) {
          emit(s, (int64_t)trow - mb.src_off[s], step);
          return;
        }
    };
    for (int64_t pos = 0; pos < mb.n_dst; ++pos)
      for (int32_t tt = 0; tt < mb.h_len[pos]; ++tt) {
        const int32_t i = mb.h_step_ptr[pos] + tt;
        const uint32_t code = mb.h_step_code[i];
        if ((int64_t)code < mb.zero_row) {
          add_row(code, i);
        } else if ((int64_t)code > mb.zero_row) {
          const int64_t k = code - mb.zero_row - 1;
          for (int32_t m = mb.h_multi_ptr[k]; m < mb.h_multi_ptr[k + 1]; ++m) add_row(mb.h_multi_rows[m], i);
        }
      }
  }, ptr, idx);
}

void lower_train_sum(int S, const int64_t* keys, const TrainMpIn& mb, std::vector<hvec<int32_t>>& ptr,
                     std::vector<hvec<int32_t>>& idx) {
  build_csrs(S, keys, [&](auto&& emit) {
    for (int64_t pos = 0; pos < mb.n_dst; ++pos)
      for (int32_t m = mb.h_msg_ptr[pos]; m < mb.h_msg_ptr[pos + 1]; ++m) {
        const uint32_t code = mb.h_msg_src[m];
        emit((int)(code >> IGN_SLOT_SHIFT), (int64_t)(code & IGN_ROW_MASK), mb.h_order[pos]);
      }
  }, ptr, idx);
}

void lower_train_attention(int S, const int64_t* keys, const TrainMpIn& mb, TrainAttn* out) {
  hvec<int32_t>& mdst = out->mdst;
  mdst.assign(mb.n_msgs, 0);
  for (int64_t pos = 0; pos < mb.n_dst; ++pos)
    for (int32_t m = mb.h_msg_ptr[pos]; m < mb.h_msg_ptr[pos + 1]; ++m) mdst[m] = mb.h_order[pos];
  std::vector<hvec<std::pair<int64_t, int32_t>>> am(S);
  for (int64_t m = 0; m < mb.n_msgs; ++m)
    am[mb.h_msg_src[m] >> IGN_SLOT_SHIFT].push_back({(int64_t)(mb.h_msg_src[m] & IGN_ROW_MASK), (int32_t)m});
  out->ptr.assign(S, hvec<int32_t>());
  out->idx.assign(S, hvec<int32_t>());
  for (int s = 0; s < S; ++s) build_csr(keys[s], am[s], out->ptr[s], out->idx[s]);
}

void lower_train_degree(const TrainMpIn& mb, hvec<float>* deg) {
  deg->assign(mb.n_dst, 0.f);
  for (int64_t pos = 0; pos < mb.n_dst; ++pos)
    (*deg)[mb.h_order[pos]] = (float)(mb.h_msg_ptr[pos + 1] - mb.h_msg_ptr[pos]);
}

void lower_row_edges(int64_t n_rows, const int32_t* row_of_edge, int64_t n_edges, hvec<int32_t>* ptr, hvec<int32_t>* idx) {
  hvec<std::pair<int64_t, int32_t>> kv(n_edges);
  for (int64_t e = 0; e < n_edges; ++e) kv[e] = {row_of_edge[e], (int32_t)e};
  build_csr(n_rows, kv, *ptr, *idx);
}

}  // namespace ign
