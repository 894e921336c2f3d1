// lower_check.h — what the stand-alone lowering checks (batch_lower_check.cpp, train_lower_check.cpp)
// share: the lowering's three external symbols, the CHECK / EQ / OK / FAILS reporting, and a batch
// desc that owns its arrays.  Each check is one translation unit plus the units under test.
#pragma once
#include <cstdarg>
#include <cstring>
#include <functional>
#include <initializer_list>

#include "../../ignnition_amd/csrc/batch_lower.h"

using namespace ign;

// the unit's three external symbols
static int g_code = 0;
static char g_msg[1024];
int ign::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return g_code = code;
}
void* ign::host_block_alloc(size_t bytes) { return std::malloc(bytes); }
void ign::host_block_free(void* p, size_t) { std::free(p); }

static int g_bad = 0;
static const char* g_case = "";
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("FAIL [%s] line %d: %s\n", g_case, __LINE__, #c);          \
      ++g_bad;                                                          \
    }                                                                   \
  } while (0)
#define EQ(v, ...) eq(#v, __LINE__, v, {__VA_ARGS__})
#define OK(e)                                                                         \
  do {                                                                                \
    const int rc_ = (e);                                                              \
    if (rc_) {                                                                        \
      printf("FAIL [%s] line %d: %s returned %d (%s)\n", g_case, __LINE__, #e, rc_, g_msg); \
      ++g_bad;                                                                        \
      return;                                                                         \
    }                                                                                 \
  } while (0)
#define FAILS(e, code, sub) fails(#e, __LINE__, (e), code, sub)

template <class V>
static void eq(const char* what, int line, const V& v, std::initializer_list<long long> want) {
  bool same = v.size() == want.size();
  size_t i = 0;
  for (long long w : want) {
    if (!same) break;
    same = (long long)v[i++] == w;
  }
  if (same) return;
  printf("FAIL [%s] line %d: %s = {", g_case, line, what);
  for (auto x : v) printf("%lld,", (long long)x);
  printf("} want {");
  for (long long w : want) printf("%lld,", w);
  printf("}\n");
  ++g_bad;
}
static inline void fails(const char* what, int line, int rc, int code, const char* sub) {
  if (rc == code && strstr(g_msg, sub)) return;
  printf("FAIL [%s] line %d: %s returned %d (%s), want %d with \"%s\"\n", g_case, line, what, rc, rc ? g_msg : "", code, sub);
  ++g_bad;
}

// a batch desc that owns its arrays, at either index width
struct Edge { int64_t s, d, q; };
struct Desc {
  int G, E, A, IL = 0;
  std::vector<int64_t> num, edges, il_len, halo;
  std::vector<std::vector<int64_t>> src, dst, seq, il;
  std::vector<std::vector<int32_t>> n32;   // the narrow copies
  std::vector<const int64_t*> psrc, pdst, pseq, pil;
  ign_batch_desc d{};
  // num: [G][E]; adj[a][g]: the graph's edges of adjacency a
  Desc(int G_, int E_, std::vector<int64_t> num_, const std::vector<std::vector<std::vector<Edge>>>& adj) : G(G_), E(E_), A((int)adj.size()), num(std::move(num_)) {
    edges.assign((size_t)G * A, 0);
    src.resize(A), dst.resize(A), seq.resize(A);
    for (int a = 0; a < A; ++a)
      for (int g = 0; g < G; ++g) {
        edges[(size_t)g * A + a] = (int64_t)adj[a][g].size();
        for (auto& e : adj[a][g]) src[a].push_back(e.s), dst[a].push_back(e.d), seq[a].push_back(e.q);
      }
  }
  // lists[i][g]: the graph's indices of interleave slot i
  Desc& interleave(const std::vector<std::vector<std::vector<int64_t>>>& lists) {
    IL = (int)lists.size();
    il.assign(IL, {});
    il_len.assign((size_t)G * IL, 0);
    for (int i = 0; i < IL; ++i)
      for (int g = 0; g < G; ++g) {
        il_len[(size_t)g * IL + i] = (int64_t)lists[i][g].size();
        il[i].insert(il[i].end(), lists[i][g].begin(), lists[i][g].end());
      }
    return *this;
  }
  const int64_t* narrow(const std::vector<int64_t>& v) {
    n32.emplace_back(v.begin(), v.end());
    n32.back().push_back(0);   // (never an empty vector's null data())
    return reinterpret_cast<const int64_t*>(n32.back().data());
  }
  const ign_batch_desc* make(int index_bytes) {
    n32.clear();
    n32.reserve(3 * A + IL);
    psrc.clear(), pdst.clear(), pseq.clear(), pil.clear();
    const bool w32 = index_bytes == 4;
    for (int a = 0; a < A; ++a) {
      psrc.push_back(w32 ? narrow(src[a]) : src[a].data());
      pdst.push_back(w32 ? narrow(dst[a]) : dst[a].data());
      pseq.push_back(w32 ? narrow(seq[a]) : seq[a].data());
    }
    for (int i = 0; i < IL; ++i) pil.push_back(w32 ? narrow(il[i]) : il[i].data());
    d = ign_batch_desc{};
    d.num_graphs = G;
    d.num_nodes = num.data();
    d.adj_edges = edges.data();
    d.adj_src = psrc.data();
    d.adj_dst = pdst.data();
    d.adj_seq = pseq.data();
    d.interleave_len = il_len.data();
    d.interleave_idx = pil.data();
    d.halo_rows = halo.empty() ? nullptr : halo.data();
    d.index_bytes = index_bytes;
    return &d;
  }
};

struct Src { int entity, adjacency, interleave; };
static MPP make_mp(int dst, int aggr, bool sorted, std::initializer_list<Src> srcs, int din = 32) {
  MPP mp{};
  mp.dst = dst;
  mp.aggr = aggr;
  mp.sorted = sorted;
  mp.din = din;
  for (auto& s : srcs) {
    ign_source_desc sd{};
    sd.entity = s.entity;
    sd.adjacency = s.adjacency;
    sd.interleave = s.interleave;
    mp.src.push_back(sd);
    mp.nn.emplace_back();
  }
  return mp;
}

static BuildMarks g_bm(false);
// shape + messages of mps[m]
static int lower_to_messages(Desc& ds, int index_bytes, const std::vector<MPP>& mps, int m, BatchShape* sh, MsgLists* ml) {
  *ml = MsgLists();   // (the engine lowers every MP into fresh lists)
  int rc = lower_batch_shape(ds.E, ds.A, ds.IL, mps, ds.make(index_bytes), sh);
  return rc ? rc : lower_messages(mps[m], *sh, ml);
}
