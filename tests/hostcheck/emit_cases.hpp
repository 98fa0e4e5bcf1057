// tests/hostcheck/emit_cases.hpp -- TEST TOOL, not part of the product.
//
// Crafted parents and deltas for the row emitters (nodestate.hpp: emit_row, emit_row_masked;
// kernels.hpp: wave_emit), shared by tests/hostcheck/emitcheck.cpp and tests/devcheck/emitcheck.hip.
// The emitters only compare records, so a case is written in RANKS: rec(v) rises strictly with v,
// a parent is a sorted list of ranks, a delta a send list of ranks in send order with its keep
// mask. Every size is derived from the protocol's kNetCap and kMaxSends (MiniTest: 4 and 2).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "../../dslabs_amd/csrc/protocols/all.hpp"

namespace emitcases {
using namespace dsl;

inline uint64_t mix(uint64_t x) {  // splitmix64's finalizer
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Strictly rising in v (v < 2^14), never 0 and never ~0; a 64-bit record varies in both words.
template <class Rec>
Rec rec(int v) {
  if constexpr (sizeof(Rec) == 8) return ((Rec)(v + 1) << 41) | (Rec)(mix((uint64_t)v) & ((1ull << 40) - 1));
  else return ((Rec)(v + 1) << 16) | (Rec)(mix((uint64_t)v) & 0x7fffu);
}

template <class P>
struct Case {
  std::string name;
  uint32_t pw[Layout<P>::kWords];
  Delta<P> d;
  bool equal_sends;  // two kept sends are equal: the emitters must report it
};

// parent: sorted distinct ranks; sends: ranks in send order (out.n of them); keep: the kept ones.
template <class P>
Case<P> make(const std::string& name, const std::vector<int>& parent, const std::vector<int>& sends, uint32_t keep,
             int node, uint64_t seed) {
  using L = Layout<P>;
  using Rec = typename P::Rec;
  Case<P> c;
  c.name = name;
  for (int o = 0; o < L::kWords; o++) c.pw[o] = 0;
  for (int o = 0; o < L::kNetCount; o++) c.pw[o] = (uint32_t)mix(seed * 1000 + (uint64_t)o);
  c.pw[L::kNetCount] = (uint32_t)parent.size();
  for (size_t q = 0; q < parent.size(); q++) Net<P>::put(c.pw, (int)q, rec<Rec>(parent[q]));
  c.d.node = node;
  for (int i = 0; i < P::kNodeWords; i++) c.d.nw[i] = (uint32_t)mix(seed * 1000 + 500 + (uint64_t)i);
  c.d.out.n = (int)sends.size();
  c.d.out.overflow = false;
  for (int i = 0; i < P::kMaxSends; i++) c.d.out.r[i] = i < (int)sends.size() ? rec<Rec>(sends[i]) : (Rec)0;
  c.d.keep = keep;
  c.equal_sends = false;
  for (size_t a = 0; a < sends.size(); a++)
    for (size_t b = a + 1; b < sends.size(); b++)
      if (((keep >> a) & 1u) && ((keep >> b) & 1u) && sends[a] == sends[b]) c.equal_sends = true;
  return c;
}

inline std::vector<int> iota_step(int n, int first, int step) {
  std::vector<int> v;
  for (int i = 0; i < n; i++) v.push_back(first + i * step);
  return v;
}

// A random case: n parent records and a send list whose unkept sends are parent records (that is
// why a handler's send is not kept), the kept ones new.
template <class P>
Case<P> random_case(const std::string& name, uint64_t seed) {
  constexpr int cap = P::kNetCap, K = P::kMaxSends;
  const int m = (int)(mix(seed) % (uint64_t)(K + 1));
  const int n = (int)(mix(seed + 1) % (uint64_t)(cap - m + 1));
  std::vector<int> all;  // distinct ranks below 4 * cap
  for (int v = 0; (int)all.size() < n + m; v++) {
    const int x = (int)(mix(seed * 77 + (uint64_t)v) % (uint64_t)(4 * cap));
    if (std::find(all.begin(), all.end(), x) == all.end()) all.push_back(x);
  }
  std::vector<int> parent(all.begin(), all.begin() + n), fresh(all.begin() + n, all.end());
  std::sort(parent.begin(), parent.end());
  std::vector<int> sends;
  uint32_t keep = 0;
  size_t f = 0;
  for (int i = 0; i < K && f < fresh.size(); i++) {
    const bool old = n > 0 && (K - i) > (int)(fresh.size() - f) && (mix(seed * 13 + (uint64_t)i) & 1);
    if (old) {
      sends.push_back(parent[mix(seed * 17 + (uint64_t)i) % (uint64_t)n]);
    } else {
      keep |= 1u << i;
      sends.push_back(fresh[f++]);
    }
  }
  return make<P>(name, parent, sends, keep, (int)(mix(seed + 5) % (uint64_t)P::kNodes), seed);
}

template <class P>
std::vector<Case<P>> crafted() {
  constexpr int cap = P::kNetCap, K = P::kMaxSends, last = P::kNodes - 1;
  const int m3 = std::min(K, 3);
  std::vector<Case<P>> out;
  // n = 0: the kept sends are the whole record array (sent in falling order)
  out.push_back(make<P>("n0", {}, iota_step(m3, 30, -7), (1u << m3) - 1u, 0, 1));
  // n + m = kNetCap: the last slot is written
  out.push_back(make<P>("full", iota_step(cap - m3, 10, 2), iota_step(m3, 11, 2 * ((cap - m3) / m3)), (1u << m3) - 1u,
                        last, 2));
  out.push_back(make<P>("full_last_new", iota_step(cap - 1, 10, 2), {5000}, 1u, 0, 3));
  // every send below / above every parent record
  out.push_back(make<P>("below_all", iota_step(cap / 2, 100, 3), iota_step(m3, 2, 3), (1u << m3) - 1u, 1 % P::kNodes, 4));
  out.push_back(make<P>("above_all", iota_step(cap / 2, 100, 3), iota_step(m3, 9000, -5), (1u << m3) - 1u, last, 5));
  // several sends in one gap of the parent's records (between its records 1 and 2 where it has 3)
  {
    const int n = std::min(cap - K, 9);
    out.push_back(make<P>("one_gap", iota_step(n, 100, 100), iota_step(K, n >= 2 ? 250 : 150, -1), (1u << K) - 1u, 0, 6));
  }
  // a keep mask with holes: bits 0, 9, 11 where the protocol has 12 sends, else the first and last
  // send; the unkept sends are parent records
  if (K >= 2 && cap >= K + 2) {
    const int n = std::min(cap - K, 20);
    uint32_t keep = K >= 12 ? ((1u << 0) | (1u << 9) | (1u << 11)) : K >= 3 ? ((1u << 0) | (1u << (K - 1))) : 2u;
    std::vector<int> sends;
    for (int i = 0; i < K; i++)
      sends.push_back(((keep >> i) & 1u) ? 95 + 10 * ((i * 7) % n) + (i & 1 ? 0 : 11) : 100 + 10 * (i % n));
    out.push_back(make<P>("keep_holes", iota_step(n, 100, 10), sends, keep, last, 7));
  }
  // all K sends kept, interleaved with the parent's records
  out.push_back(make<P>("all_sends", iota_step(cap - K, 10, 10), iota_step(K, 5 + 10 * (K - 1), -10), (1u << K) - 1u, 0, 8));
  // nothing kept: only the node's words and the count change
  out.push_back(make<P>("no_new", iota_step(cap / 2, 10, 10), {10}, 0u, last, 9));
  // the changed node first and last
  out.push_back(make<P>("node_first", iota_step(cap / 2, 10, 10), {15}, 1u, 0, 10));
  out.push_back(make<P>("node_last", iota_step(cap / 2, 10, 10), {15}, 1u, last, 11));
  // two equal kept sends: reported, never a silently wrong row
  if (K >= 2) {
    out.push_back(make<P>("equal_sends", iota_step(cap / 2, 10, 10), {15, 15}, 3u, 0, 12));
    if (K >= 3 && cap >= 4) out.push_back(make<P>("equal_sends_apart", iota_step(cap / 2, 10, 10), {95, 15, 95}, 7u, 0, 13));
  }
  for (int i = 0; i < 8; i++) out.push_back(random_case<P>("random" + std::to_string(i), 100 + (uint64_t)i));
  return out;
}

}  // namespace emitcases
