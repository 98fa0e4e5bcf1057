// nodestate.hpp -- generic packed search state + incremental set fingerprint.
//
// A packed state is [kNodes x kNodeWords node words][net count][records, sorted, distinct].
// Node words hold a node's fields and its timer queue; the network is the SET of sent messages
// (delivery never removes, duplicates collapse: SearchState.java:71, :300-301).
//
// Protocols are node-local, as DSLabs handlers are (F/Node.java:387-562): a handler sees only
// its node's words and the delivered message / fired timer, updates the words and emits sends.
// A successor is therefore a DELTA of its parent: one node's new words + a short send list.
//
// Fingerprint (128 bit): the XOR over nodes i of H_node(i, words_i) and over the network's
// records r of H_msg(r), with H = MurmurHash3_x64_128 block/finalizer structure under domain
// seeds. It is order-independent over the record set, so
//     fp(successor) = fp(parent) ^ H_node(i, old) ^ H_node(i, new) ^ XOR_{r new to the set} H_msg(r)
// is computed without materializing the successor. For n distinct states the chance that two
// share a fingerprint is ~ n^2 / 2^129 (each pair of distinct states differs in a non-empty
// set of hashed components).
#pragma once
#include <string>
#include <type_traits>

#include "common.hpp"
#include "fingerprint.hpp"

namespace dsl {

template <class P>
struct Layout {
  using Rec = typename P::Rec;
  static constexpr int kRecWords = (int)(sizeof(Rec) / 4);
  static constexpr int kNetCount = P::kNodes * P::kNodeWords;
  static constexpr int kRecBase = ((kNetCount + 1 + kRecWords - 1) / kRecWords) * kRecWords;
  static constexpr int kWords = ((kRecBase + P::kNetCap * kRecWords) + 3) / 4 * 4;
};

template <class P>
using StateOf = Packed<Layout<P>::kWords>;

template <class P>
struct Net {
  using L = Layout<P>;
  using Rec = typename P::Rec;
  static DSL_HD int size(const uint32_t* w) { return (int)w[L::kNetCount]; }
  static DSL_HD Rec at(const uint32_t* w, int i) {
    if constexpr (sizeof(Rec) == 8) {
      return (Rec)w[L::kRecBase + 2 * i] | ((Rec)w[L::kRecBase + 2 * i + 1] << 32);
    } else {
      return (Rec)w[L::kRecBase + i];
    }
  }
  static DSL_HD void put(uint32_t* w, int i, Rec r) {
    if constexpr (sizeof(Rec) == 8) {
      w[L::kRecBase + 2 * i] = (uint32_t)r;
      w[L::kRecBase + 2 * i + 1] = (uint32_t)((uint64_t)r >> 32);
    } else {
      w[L::kRecBase + i] = (uint32_t)r;
    }
  }
  static DSL_HD bool contains(const uint32_t* w, Rec r) {
    int lo = 0, hi = size(w);
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      Rec x = at(w, mid);
      if (x == r) return true;
      if (x < r) lo = mid + 1; else hi = mid;
    }
    return false;
  }
  // 0 inserted, 1 present, -1 overflow
  static DSL_HD int insert(uint32_t* w, Rec r) {
    int n = size(w), lo = 0, hi = n;
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      if (at(w, mid) < r) lo = mid + 1; else hi = mid;
    }
    if (lo < n && at(w, lo) == r) return 1;
    if (n >= P::kNetCap) return -1;
    for (int j = n; j > lo; j--) put(w, j, at(w, j - 1));
    put(w, lo, r);
    w[L::kNetCount] = (uint32_t)(n + 1);
    return 0;
  }
};

// P::kNetPreds: some predicate of P reads the network (StatePredicate.containsMessageMatching),
// so the judge's view must carry the successor's new records.
template <class P, class = void>
struct NetPreds : std::false_type {};
template <class P>
struct NetPreds<P, std::void_t<decltype(P::kNetPreds)>> : std::integral_constant<bool, P::kNetPreds> {};
// P::kSendsDistinct: no handler of P sends one record twice in one step (tests/hostcheck checks
// it on every explored step), so Sender needs no duplicate check.
template <class P, class = void>
struct SendsDistinct : std::false_type {};
template <class P>
struct SendsDistinct<P, std::void_t<decltype(P::kSendsDistinct)>> : std::integral_constant<bool, P::kSendsDistinct> {};

// Sends emitted by one handler invocation (duplicates collapse, as in the network set).
// Every access to r[] uses a compile-time index (fully unrolled loops predicated on i < n), so
// the list lives in VGPRs; a dynamically indexed per-lane array would be placed in scratch and
// every send would pay a memory round trip.
template <class P>
struct Sender {
  using Rec = typename P::Rec;
  static constexpr int K = P::kMaxSends;
  int n = 0;
  bool overflow = false;
  Rec r[K];
  DSL_HD void send(Rec x) {
    if constexpr (!SendsDistinct<P>::value) {
      bool dup = false;
#pragma unroll
      for (int i = 0; i < K; i++)
        if (i < n && r[i] == x) dup = true;
      if (dup) return;
    }
    if (n >= K) {
      overflow = true;
      return;
    }
#pragma unroll
    for (int i = 0; i < K; i++) {
      if (wave_none(i <= n)) break;  // every sending lane's slot is behind
      r[i] = keep_value(i == n ? x : r[i]);
    }
    n++;
  }
};

// Read access to a state's node words (what predicates and handlers see).
struct NodeView {
  const uint32_t* base;     // node words of the parent state
  int nw;                   // words per node
  int changed;              // node replaced by `over` (-1: none)
  const uint32_t* over;
  // network predicates (P::kNetPreds): the state's records are the parent row's (base is a whole
  // row) plus `nsends` new records of type P::Rec at `sends`
  const void* sends = nullptr;
  int nsends = 0;
  // the dropped network (DevSettings::dropped, set by judge_view): part of network() for
  // predicates, never an event
  const void* dropped = nullptr;
  int ndropped = 0;
  // the generic network leaves (DSL_PRED_NET): bit i = a record NEW to the parent's set satisfies
  // network leaf i (DevPred::pad). The kernels compute it from the delta's registers
  // (delta_net_hits), host code from `sends` (judge_view); 0 for a materialized row
  uint32_t net_hits = 0;
  // bit i = a record of the row at `base`, or a dropped record, satisfies network leaf i
  // (row_net_hits); filled in only when the judge needs it (net_needs_row)
  uint32_t row_hits = 0;
  DSL_HD const uint32_t* node(int i) const { return i == changed ? over : base + i * nw; }
};

// Any record of the viewed state's network() -- parent records, the view's new records and the
// dropped records (SearchState.network() = network + droppedNetwork, SearchState.java:153-157;
// StatePredicate.containsMessageMatching reads it, T/StatePredicate.java:146-149) -- satisfying f.
template <class P, class F>
DSL_HD bool view_any_record(const NodeView& v, F f) {
  const int n = Net<P>::size(v.base);
  for (int j = 0; j < n; j++)
    if (f(Net<P>::at(v.base, j))) return true;
  const auto* r = static_cast<const typename P::Rec*>(v.sends);
  for (int j = 0; j < v.nsends; j++)
    if (f(r[j])) return true;
  const auto* x = static_cast<const typename P::Rec*>(v.dropped);
  for (int j = 0; j < v.ndropped; j++)
    if (f(x[j])) return true;
  return false;
}

// ---- fingerprint ------------------------------------------------------------------------------
DSL_HD Fp fp_xor(Fp a, Fp b) { return Fp{a.hi ^ b.hi, a.lo ^ b.lo}; }

template <int NW>
DSL_HD Fp hash_words(const uint32_t* w, uint64_t seed) {
  const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
  uint64_t h1 = seed ^ 0x9368e53c2f6af274ULL, h2 = seed ^ 0x586dcd208f7cd3fdULL;
#pragma unroll
  for (int i = 0; i < NW; i += 4) {
    const uint64_t k1 = (uint64_t)w[i] | ((uint64_t)(i + 1 < NW ? w[i + 1] : 0u) << 32);
    const uint64_t k2 = (uint64_t)(i + 2 < NW ? w[i + 2] : 0u) | ((uint64_t)(i + 3 < NW ? w[i + 3] : 0u) << 32);
    uint64_t a = k1 * c1;
    a = rotl64(a, 31) * c2;
    h1 ^= a;
    h1 = rotl64(h1, 27) + h2;
    h1 = h1 * 5 + 0x52dce729;
    uint64_t b = k2 * c2;
    b = rotl64(b, 33) * c1;
    h2 ^= b;
    h2 = rotl64(h2, 31) + h1;
    h2 = h2 * 5 + 0x38495ab5;
  }
  h1 ^= (uint64_t)(NW * 4);
  h2 ^= (uint64_t)(NW * 4);
  h1 += h2;
  h2 += h1;
  h1 = fmix64(h1);
  h2 = fmix64(h2);
  h1 += h2;
  h2 += h1;
  return Fp{h1, h2};
}

template <class P>
DSL_HD Fp node_hash(int i, const uint32_t* w) {
  return hash_words<P::kNodeWords>(w, 0x5EED00000000ull + (uint64_t)i);
}

template <class P>
DSL_HD Fp msg_hash(typename P::Rec r) {
  uint32_t w[2] = {(uint32_t)(uint64_t)r, (uint32_t)((uint64_t)r >> 32)};
  return hash_words<2>(w, 0x0E7A5E7ull);
}

template <class P>
DSL_HD Fp full_fingerprint(const uint32_t* w) {
  Fp f{0, 0};
  for (int i = 0; i < P::kNodes; i++) f = fp_xor(f, node_hash<P>(i, w + i * P::kNodeWords));
  const int n = Net<P>::size(w);
  for (int j = 0; j < n; j++) f = fp_xor(f, msg_hash<P>(Net<P>::at(w, j)));
  return f;
}

// ---- events -------------------------------------------------------------------------------------
// Enabled events of a state (SearchState.events, SearchState.java:226-252): every network record
// whose (from, to) passes shouldDeliver and whose destination exists, in record order; then for
// every node with deliverTimers(node), its deliverable timers (TimerQueue.deliverable()).
template <class P>
DSL_HD int count_events(const uint32_t* w, const typename P::Params& prm, const DevSettings& set) {
  int n = 0;
  const int cnt = Net<P>::size(w);
  const int nodes = P::num_nodes(prm);
  if (set.all_deliver) {
    n = cnt;
  } else {
    for (int j = 0; j < cnt; j++) {
      const auto r = Net<P>::at(w, j);
      n += should_deliver(set, P::rec_from(r), P::rec_to(r));
    }
  }
  for (int i = 0; i < nodes; i++)
    if (deliver_timers(set, i)) n += P::num_timer_events(i, w + i * P::kNodeWords, prm);
  return n;
}

// Locates event k: returns >= 0 = record index, or -1 - (node * 256 + j) for timer j of node.
template <class P>
DSL_HD int locate_event(const uint32_t* w, const typename P::Params& prm, const DevSettings& set, int k) {
  const int cnt = Net<P>::size(w);
  if (set.all_deliver) {
    if (k < cnt) return k;
    k -= cnt;
  } else {
    for (int j = 0; j < cnt; j++) {
      const auto r = Net<P>::at(w, j);
      if (should_deliver(set, P::rec_from(r), P::rec_to(r)) && k-- == 0) return j;
    }
  }
  const int nodes = P::num_nodes(prm);
  for (int i = 0; i < nodes; i++) {
    if (!deliver_timers(set, i)) continue;
    const int t = P::num_timer_events(i, w + i * P::kNodeWords, prm);
    if (k < t) return -1 - (i * 256 + k);
    k -= t;
  }
  return INT32_MIN;
}

// Handler classes (k_level sorts a chunk's work items by class, so a wavefront mostly runs one
// handler): messages [0, kMsgClasses) by P::msg_class; timers from kMsgClasses on, one class, or
// TimerClasses<P> of them when the protocol splits its timer handlers by node kind
// (P::kTimerClasses + P::timer_class(node): Multi-Paxos's server Tick and client ClientTimer,
// which a wave of mixed timer items would otherwise both run); last the skip class (NoopFilter).
template <class P, class = void>
struct TimerClasses : std::integral_constant<int, 1> {
  static DSL_HD int of(int, const typename P::Params&) { return 0; }
};
template <class P>
struct TimerClasses<P, std::void_t<decltype(P::kTimerClasses)>> : std::integral_constant<int, P::kTimerClasses> {
  static DSL_HD int of(int node, const typename P::Params& prm) { return P::timer_class(node, prm); }
};
template <class P>
struct Classes {
  static constexpr int kTimer0 = P::kMsgClasses;
  static constexpr int kSkip = P::kMsgClasses + TimerClasses<P>::value;
  static constexpr int kCount = kSkip + 1;
  static_assert(P::kMsgClasses >= 1 && kCount <= 16, "at most 16 handler classes, the skip class included");
};

// Events whose handler surely changes nothing: a protocol may provide
//   static bool surely_noop(int node, const uint32_t* w, Rec r, const Params&)
//   static bool surely_noop_timer(int node, const uint32_t* w, int timer, const Params&)
// (w = the whole state row) returning true only when the event surely returns STEP_OK with the
// node's words unchanged and every send already in the network (the successor is the parent;
// `false` whenever unsure). k_level counts such an event as a successor (Search.java:481-485: it
// is generated, then found in the visited set) without running its handler; tests/hostcheck
// checks the implication on every explored event. event_class_skip returns Classes<P>::kSkip for them.
template <class P, class = void>
struct NoopFilter {
  static DSL_HD bool msg(int, const uint32_t*, typename P::Rec, const typename P::Params&) { return false; }
};
template <class P>
struct NoopFilter<P, std::void_t<decltype(&P::surely_noop)>> {
  static DSL_HD bool msg(int i, const uint32_t* w, typename P::Rec r, const typename P::Params& prm) {
    return P::surely_noop(i, w, r, prm);
  }
};
template <class P, class = void>
struct NoopTimerFilter {
  static DSL_HD bool timer(int, const uint32_t*, int, const typename P::Params&) { return false; }
};
template <class P>
struct NoopTimerFilter<P, std::void_t<decltype(&P::surely_noop_timer)>> {
  static DSL_HD bool timer(int i, const uint32_t* w, int t, const typename P::Params& prm) {
    return P::surely_noop_timer(i, w, t, prm);
  }
};

template <class P>
DSL_HD int event_class_skip(const uint32_t* w, const typename P::Params& prm, const DevSettings& set, int k,
                            int* located = nullptr) {
  const int e = locate_event<P>(w, prm, set, k);
  if (located) *located = e;  // k_level keeps it for delta_step_located (no second walk)
  if (e < 0) {
    if (e == INT32_MIN) return Classes<P>::kTimer0;
    const int x = -1 - e;
    return NoopTimerFilter<P>::timer(x >> 8, w, x & 255, prm) ? Classes<P>::kSkip
                                                                : Classes<P>::kTimer0 + TimerClasses<P>::of(x >> 8, prm);
  }
  const auto r = Net<P>::at(w, e);
  const int i = P::rec_to(r);
  if (i < P::num_nodes(prm) && NoopFilter<P>::msg(i, w, r, prm)) return Classes<P>::kSkip;
  return P::msg_class(r);
}

// A successor as a delta of its parent: one node's new words and the handler's sends (distinct);
// bit i of `keep` marks send i as new to the parent's network set. The records the successor adds
// are exactly the kept sends; they stay in send order (nothing is moved or sorted), and every
// consumer that needs the merged order ranks them itself (delta_rank).
template <class P>
struct Delta {
  int node;
  uint32_t nw[P::kNodeWords];
  Sender<P> out;
  uint32_t keep;
};

template <class P>
DSL_HD int delta_new_count(const Delta<P>& d) { return __builtin_popcount(d.keep); }

// Marks the sends that are not already in the parent's network set (canonical successor: the
// set union). No reordering: the send list stays where the handler wrote it, in VGPRs.
// Membership by a fixed-trip lower bound over the sorted records (log2(kNetCap) + 1 dependent LDS
// reads, selects instead of a data-dependent loop: C5 d12 -1.5 % against Net::contains).
template <class P>
DSL_HD bool net_contains_fixed(const uint32_t* w, int n, typename P::Rec r) {
  int pos = 0;
#pragma unroll
  for (int step = 1 << (31 - __builtin_clz((unsigned)P::kNetCap)); step > 0; step >>= 1) {
    const int q = pos + step;
    pos = (q <= n && Net<P>::at(w, q - 1) < r) ? q : pos;
  }
  return pos < n && Net<P>::at(w, pos) == r;
}

template <class P>
DSL_HD void canon_sends(const uint32_t* w, Delta<P>& d) {
  constexpr int K = P::kMaxSends;
  const int n = d.out.n;
  uint32_t keep = 0;
  const int nr = Net<P>::size(w);
#pragma unroll
  for (int i = 0; i < K; i++) {
    if (wave_none(i < n)) break;
    if (i < n && !net_contains_fixed<P>(w, nr, d.out.r[i])) keep |= 1u << i;
  }
  d.keep = keep;
}

// The kept sends, compacted in send order into out[]; returns their number (host code and LDS views).
template <class P>
DSL_HD int delta_sends(const Delta<P>& d, typename P::Rec* out) {
  int m = 0;
  for (int i = 0; i < P::kMaxSends; i++)
    if ((d.keep >> i) & 1u) out[m++] = d.out.r[i];
  return m;
}

// Applies event k of parent w: fills the delta (its send list canonical); returns a StepRc.
template <class P>
DSL_HD int delta_step_located(const uint32_t* w, int e, Delta<P>& d, const typename P::Params& prm,
                              const DevSettings& set);
template <class P>
DSL_HD int delta_step(const uint32_t* w, int k, Delta<P>& d, const typename P::Params& prm, const DevSettings& set) {
  return delta_step_located<P>(w, locate_event<P>(w, prm, set, k), d, prm, set);
}
// The same for an event already located (locate_event's code e).
template <class P>
DSL_HD int delta_step_located(const uint32_t* w, int e, Delta<P>& d, const typename P::Params& prm,
                              const DevSettings& set) {
  if (e == INT32_MIN) return STEP_NULL;
  d.out.n = 0;
  d.out.overflow = false;
  d.keep = 0;
  int rc;
  if (e >= 0) {
    const auto r = Net<P>::at(w, e);
    d.node = P::rec_to(r);
    if (d.node >= P::num_nodes(prm)) return STEP_NULL;
    for (int i = 0; i < P::kNodeWords; i++) d.nw[i] = w[d.node * P::kNodeWords + i];
    rc = P::on_message(d.node, d.nw, r, d.out, prm);
  } else {
    const int x = -1 - e;
    d.node = x >> 8;
    for (int i = 0; i < P::kNodeWords; i++) d.nw[i] = w[d.node * P::kNodeWords + i];
    rc = P::on_timer(d.node, d.nw, x & 255, d.out, prm);
  }
  if (d.out.overflow && rc == STEP_OK) rc = STEP_OVERFLOW;
  if (rc == STEP_OK) canon_sends<P>(w, d);
  else d.keep = (1u << d.out.n) - 1u;  // an exceptional state keeps what was sent before the throw
  return rc;
}

// Successor fingerprint from the parent's: node delta + the sends not already in the set.
template <class P>
DSL_HD Fp delta_fingerprint(const uint32_t* w, Fp parent, const Delta<P>& d) {
  Fp f = fp_xor(parent, node_hash<P>(d.node, w + d.node * P::kNodeWords));
  f = fp_xor(f, node_hash<P>(d.node, d.nw));
#pragma unroll
  for (int j = 0; j < P::kMaxSends; j++) {
    if (wave_none((d.keep >> j) != 0u)) break;
    if ((d.keep >> j) & 1u) f = fp_xor(f, msg_hash<P>(d.out.r[j]));  // the records new to the set
  }
  return f;
}

// The same from the parent's fingerprint with the changed node's old hash already removed
// (k_level caches the parents' node hashes in LDS).
template <class P>
DSL_HD Fp delta_fingerprint_cached(Fp parent_without_node, const Delta<P>& d) {
  Fp f = fp_xor(parent_without_node, node_hash<P>(d.node, d.nw));
#pragma unroll
  for (int j = 0; j < P::kMaxSends; j++) {
    if (wave_none((d.keep >> j) != 0u)) break;
    if ((d.keep >> j) & 1u) f = fp_xor(f, msg_hash<P>(d.out.r[j]));
  }
  return f;
}

// Enabled events of the successor, from the parent's count and the delta: the changed node's
// timer events are replaced, records new to the set add their deliverable ones.
template <class P>
DSL_HD int delta_event_count(const uint32_t* w, int parent_events, const Delta<P>& d, const typename P::Params& prm,
                             const DevSettings& set) {
  int n = parent_events;
  if (deliver_timers(set, d.node))
    n += P::num_timer_events(d.node, d.nw, prm) - P::num_timer_events(d.node, w + d.node * P::kNodeWords, prm);
#pragma unroll
  for (int j = 0; j < P::kMaxSends; j++) {  // the records new to the set
    if (wave_none((d.keep >> j) != 0u)) break;
    if ((d.keep >> j) & 1u) {
      const auto r = d.out.r[j];
      if (set.all_deliver || should_deliver(set, P::rec_from(r), P::rec_to(r))) n++;
    }
  }
  return n;
}

// ---- sleep sets ---------------------------------------------------------------------
// Two deliveries to different nodes commute: parent G with message events A and B generates G+A
// and G+B, and both later generate G+A+B. A frontier state P therefore carries a CREATOR record of
// how it was first inserted -- the event Cr that made it from its recorded parent G, the node c
// whose words Cr changed, and which of P's records are new against G -- and, when P is expanded,
// a message event E (record r, destination e) SLEEPS when all of these hold:
//   1. P has a creator record;
//   2. r was already in G's network (its slot is not marked new);
//   3. e != c, and e is an existing node;
//   4. Cr is a timer event, or sleep_key(r) < sleep_key(rec(Cr)) (a tie: nobody sleeps).
// A sleeping event is counted as a successor and never run: G+E exists at P's depth, still has Cr
// enabled and reaches the same state, and the key rises strictly along such a chain, so some
// state of the frontier runs the event. Timer events never sleep. The rule needs every frontier
// state expanded with every record deliverable: the host switches it off (no creator is read)
// for settings with a prune or a dropped link and for more than one shard.
// A protocol opts out with `static constexpr bool kSleepSets = false`; one whose network holds
// more than 64 records is out (the new-record mask is one 64-bit word).
template <class P, class = void>
struct SleepSets : std::integral_constant<bool, (P::kNetCap <= 64)> {};
template <class P>
struct SleepSets<P, std::void_t<decltype(P::kSleepSets)>>
    : std::integral_constant<bool, (P::kSleepSets && P::kNetCap <= 64)> {};

// What the settings must allow (the host decides once per search; the engine adds: one shard):
// every record deliverable, and no prune -- a pruned state is not expanded, and the argument
// needs every state of a level expanded. Goals and invariants end the search at their level.
template <class P>
inline bool sleep_sets_apply(const DevSettings& set) {
  return SleepSets<P>::value && set.all_deliver != 0 && set.n_prune == 0;
}

// The creator word: has | timer | node c (6 bits) | the 24-bit key of Cr's record. 0 = none.
constexpr uint32_t kCrHas = 1u << 31, kCrTimer = 1u << 30, kCrKeyMask = (1u << 24) - 1u;
constexpr int kCrNodeShift = 24;
// A fixed function of the record value alone.
template <class Rec>
DSL_HD uint32_t sleep_key(Rec r) {
  const uint64_t x = (uint64_t)r;
  return ((((uint32_t)x ^ ((uint32_t)(x >> 32) * 0x9E3779B1u)) * 0x85EBCA6Bu) >> 8) & kCrKeyMask;
}

// The creator word of a successor made by located event e of parent row w, which changed `node`.
template <class P>
DSL_HD uint32_t creator_word(const uint32_t* w, int e, int node) {
  return kCrHas | ((uint32_t)node << kCrNodeShift) |
         (e >= 0 ? sleep_key<typename P::Rec>(Net<P>::at(w, e)) : kCrTimer);
}

// The slots of the merged record array that the sends of d marked in `keep` take (parent row w;
// at most 64 records): a kept send's slot is its rank, the parent's records below it plus the kept
// sends below it, as emit_row places it. Calls visit(i, slot, record) for every kept send i (i is
// a compile-time constant after unrolling: the send list stays in VGPRs) and returns the mask of
// the slots. Two equal kept sends share a slot: the mask then has fewer bits than `keep`.
// One copy of the rule for creator_record, emit_row_masked and the kernels' wave_emit. On the
// device every lane of the wave calls it, a lane without a row with keep = 0 (it reads nothing).
template <class P, class V>
DSL_HD uint64_t delta_new_slots(const uint32_t* w, const Delta<P>& d, uint32_t keep, V visit) {
  using Rec = typename P::Rec;
  const int n = keep ? Net<P>::size(w) : 0;
  uint64_t m = 0;
#pragma unroll
  for (int i = 0; i < P::kMaxSends; i++) {
    if (wave_none((keep >> i) != 0u)) break;  // no lane keeps a later send
    if ((keep >> i) & 1u) {
      const Rec r = d.out.r[i];
      int pos = 0;  // the parent's records below r: a fixed-trip lower bound (net_contains_fixed)
#pragma unroll
      for (int step = 1 << (31 - __builtin_clz((unsigned)P::kNetCap)); step > 0; step >>= 1) {
        const int q = pos + step;
        pos = (q <= n && Net<P>::at(w, q - 1) < r) ? q : pos;
      }
#pragma unroll
      for (int j = 0; j < P::kMaxSends; j++)
        if (j != i) pos += (((keep >> j) & 1u) && d.out.r[j] < r) ? 1 : 0;
      m |= 1ull << (pos & 63);
      visit(i, pos, r);
    }
  }
  return m;
}

// The creator record of the successor (parent row w, located event e, delta d): the word, and the
// mask of the merged record array's slots that the kept sends take (delta_new_slots).
template <class P>
DSL_HD void creator_record(const uint32_t* w, int e, const Delta<P>& d, uint32_t* cw, uint64_t* cm) {
  *cm = delta_new_slots<P>(w, d, d.keep, [](int, int, typename P::Rec) {});
  *cw = creator_word<P>(w, e, d.node);
}

// The branch-free test: record `idx` of the row (value r, destination `to`; `nodes` exist) sleeps
// under the row's creator (cw, cm).
template <class Rec>
DSL_HD bool sleeping_rec(uint32_t cw, uint64_t cm, int idx, Rec r, int to, int nodes) {
  const bool old = !((cm >> (idx & 63)) & 1ull);
  const bool other = to != (int)((cw >> kCrNodeShift) & 63u) && to < nodes;
  const bool lower = (cw & kCrTimer) != 0u || sleep_key<Rec>(r) < (cw & kCrKeyMask);
  return (cw & kCrHas) != 0u && old && other && lower;
}
template <class P>
DSL_HD bool sleeping(const uint32_t* w, uint32_t cw, uint64_t cm, int idx, const typename P::Params& prm) {
  const auto r = Net<P>::at(w, idx);
  return sleeping_rec<typename P::Rec>(cw, cm, idx, r, P::rec_to(r), P::num_nodes(prm));
}

// ---- merged-row emission ----------------------------------------------------------------------
// The successor row = parent row with one node's words replaced and the canonical sends merged
// into the sorted record array. The kernels write it lane-parallel (kernels.hpp: wave_emit):
// header word o is the parent's word o, the replaced node's word, or the new record count; the
// merged record array is written by element: the parent's record q goes to slot q + (new records
// below it), a new record r to slot (parent records below r) + (new records below r) -- its rank
// among all the elements, as the records are distinct -- and the slots past n + m are zero.
// emit_row restates exactly that element-wise rule on the host (tests/hostcheck checks it
// against materialize(), which inserts the records one by one). For a protocol of at most 64
// records wave_emit writes the same row from the mask of the new records' slots
// (emit_row_masked below, held against emit_row by tests/hostcheck/emitcheck.cpp).
template <class P>
DSL_HD bool emit_row(const uint32_t* pw, const Delta<P>& d, uint32_t* out) {
  using L = Layout<P>;
  using Rec = typename P::Rec;
  Rec s[P::kMaxSends];
  const int n = Net<P>::size(pw), m = delta_sends<P>(d, s);
  if (n + m > P::kNetCap) return false;
  for (int o = 0; o < L::kRecBase; o++) {
    uint32_t v = o < L::kNetCount ? pw[o] : o == L::kNetCount ? (uint32_t)(n + m) : 0u;
    const int rel = o - d.node * P::kNodeWords;
    if (rel >= 0 && rel < P::kNodeWords) v = d.nw[rel];
    out[o] = v;
  }
  for (int o = L::kRecBase; o < L::kWords; o++) out[o] = 0u;
  auto put = [&](int slot, Rec r) {
    if constexpr (sizeof(Rec) == 8) {
      out[L::kRecBase + 2 * slot] = (uint32_t)r;
      out[L::kRecBase + 2 * slot + 1] = (uint32_t)((uint64_t)r >> 32);
    } else {
      out[L::kRecBase + slot] = (uint32_t)r;
    }
  };
  for (int q = 0; q < n; q++) {
    const Rec e = Net<P>::at(pw, q);
    int rk = q;
    for (int i = 0; i < m; i++) rk += s[i] < e;
    put(rk, e);
  }
  for (int i = 0; i < m; i++) {
    int pos = 0;
    for (int q = 0; q < n; q++) pos += Net<P>::at(pw, q) < s[i];
    for (int j = 0; j < m; j++) pos += s[j] < s[i];
    put(pos, s[i]);
  }
  return true;
}

// Which rule wave_emit writes a protocol's rows by: the mask rule (below) where the record array
// fits one 64-bit mask, unless the protocol opts out with `static constexpr bool kMaskEmit = false`
// (PB: its steps add at most one new record, so the rank rule's per-send loop is short, and the
// mask rule's prepass ran the C4 search 1 % slower, profiles/emit_mask_ab.txt).
template <class P, class = void>
struct MaskEmit : std::integral_constant<bool, (P::kNetCap <= 64)> {};
template <class P>
struct MaskEmit<P, std::void_t<decltype(P::kMaskEmit)>>
    : std::integral_constant<bool, (P::kMaskEmit && P::kNetCap <= 64)> {};

// The mask rule: what wave_emit executes for a protocol of at most 64 records, restated
// element-wise (tests/hostcheck/emitcheck.cpp holds it against emit_row on every successor).
// M = delta_new_slots' mask, m its bit count: a kept send is stored at its slot; every other slot
// s < n + m takes the parent's record s - (bits of M below s). *mask = M; *collision = two kept
// sends were equal (M has fewer bits than keep: the caller raises an error, the row is not used).
template <class P>
DSL_HD bool emit_row_masked(const uint32_t* pw, const Delta<P>& d, uint32_t* out, uint64_t* mask, bool* collision) {
  using L = Layout<P>;
  using Rec = typename P::Rec;
  static_assert(P::kNetCap <= 64, "the new-record mask is one 64-bit word");
  const int n = Net<P>::size(pw);
  if (n + delta_new_count<P>(d) > P::kNetCap) return false;
  for (int o = L::kRecBase; o < L::kWords; o++) out[o] = 0u;
  const uint64_t M = delta_new_slots<P>(pw, d, d.keep, [&](int, int slot, Rec r) { Net<P>::put(out, slot, r); });
  const int m = __builtin_popcountll(M);
  for (int o = 0; o < L::kRecBase; o++) {
    uint32_t v = o < L::kNetCount ? pw[o] : o == L::kNetCount ? (uint32_t)(n + m) : 0u;
    const int rel = o - d.node * P::kNodeWords;
    if (rel >= 0 && rel < P::kNodeWords) v = d.nw[rel];
    out[o] = v;
  }
  for (int s = 0; s < n + m; s++) {
    if ((M >> s) & 1ull) continue;
    Net<P>::put(out, s, Net<P>::at(pw, s - __builtin_popcountll(M & ((1ull << s) - 1ull))));
  }
  *mask = M;
  *collision = m != delta_new_count<P>(d);
  return true;
}

// Materializes the successor (parent w + delta) into out; false on network overflow.
template <class P>
DSL_HD bool materialize(const uint32_t* w, const Delta<P>& d, uint32_t* out) {
  for (int i = 0; i < Layout<P>::kWords; i++) out[i] = w[i];
  for (int i = 0; i < P::kNodeWords; i++) out[d.node * P::kNodeWords + i] = d.nw[i];
  for (int j = 0; j < d.out.n; j++)
    if (((d.keep >> j) & 1u) && Net<P>::insert(out, d.out.r[j]) < 0) return false;
  return true;
}

// Whole-state step (host-side trace replay, initial states).
template <class P>
DSL_HD int full_step(const uint32_t* w, int k, uint32_t* out, const typename P::Params& prm, const DevSettings& set) {
  Delta<P> d;
  int rc = delta_step<P>(w, k, d, prm, set);
  if (rc == STEP_NULL) return rc;
  if (!materialize<P>(w, d, out)) return STEP_OVERFLOW;
  return rc;
}

// Initial state: every node added and init()-ed in address order (SearchState.setupNode).
template <class P>
DSL_HD bool init_state(uint32_t* w, const typename P::Params& prm) {
  for (int i = 0; i < Layout<P>::kWords; i++) w[i] = 0;
  for (int i = 0; i < P::num_nodes(prm); i++) {
    Sender<P> out;
    P::init_node(i, w + i * P::kNodeWords, out, prm);
    if (out.overflow) return false;
    for (int j = 0; j < out.n; j++)
      if (Net<P>::insert(w, out.r[j]) < 0) return false;
  }
  return true;
}

// Decodes event k of state w for traces (MessageEnvelope / TimerEnvelope fields).
template <class P>
void describe_event(const uint32_t* w, int k, const typename P::Params& prm, const DevSettings& set, dsl_event* e) {
  *e = dsl_event{};
  const int x = locate_event<P>(w, prm, set, k);
  if (x == INT32_MIN) return;
  if (x >= 0) {
    P::describe_message(Net<P>::at(w, x), e);
  } else {
    const int y = -1 - x, node = y >> 8;
    P::describe_timer(node, w + node * P::kNodeWords, y & 255, prm, e);
  }
}

// Incremental predicate evaluation (judge_view below): a leaf that reads neither the changed node
// nor the network keeps the parent's value. A leaf reading the changed node is also unchanged
// when the words it reads are: the
// protocol's pred_same(pr, old, new) says so (e.g. Multi-Paxos LOGS_CONSISTENT reads only the
// servers' log words); without one, the node's words must all be equal.
template <int N>
DSL_HD bool same_words(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < N; i++) d |= a[i] ^ b[i];
  return d == 0;
}
template <class P, class = void>
struct PredSame {
  static DSL_HD bool same(const DevPred&, const uint32_t* a, const uint32_t* b) { return same_words<P::kNodeWords>(a, b); }
};
template <class P>
struct PredSame<P, std::void_t<decltype(&P::pred_same)>> {
  static DSL_HD bool same(const DevPred& pr, const uint32_t* a, const uint32_t* b) { return P::pred_same(pr, a, b); }
};

// ---- the generic field leaf (DSL_PRED_FIELD, include/dslabs_hip.h) -------------------------------
// An unsigned comparison of a bit field of one node with a constant or with a second field,
// judged here for every protocol (P::eval never sees the id). The word is read with a run-time
// index through the view's pointers: in every kernel both the parent row and the changed node's
// words (NodeView::over) are memory (LDS; kernels.hpp copies the delta's words there for the
// judge), so this is one indexed read, not an index into a per-lane register array.
DSL_HD uint32_t field_leaf_read(const NodeView& v, uint32_t desc) {
  const int bit = DSL_FIELD_BIT(desc), width = DSL_FIELD_WIDTH(desc);
  const uint32_t x = v.node(DSL_FIELD_NODE(desc))[bit >> 5] >> (bit & 31);
  return width >= 32 ? x : x & ((1u << width) - 1u);  // no 1u << 32
}
DSL_HD int eval_field_leaf(const DevPred& pr, const NodeView& v) {
  const uint32_t a = field_leaf_read(v, (uint32_t)pr.arg0);
  const uint32_t b = (pr.pad & kFieldRhsIsField) ? field_leaf_read(v, (uint32_t)pr.arg1) : (uint32_t)pr.arg1;
  // DSL_CMP_*: bits 1-2 pick ==, < or <=; bit 0 negates (NE, GE, GT)
  const uint32_t c = pr.pad & 7u;
  const bool base = (c >> 1) == 0 ? a == b : (c >> 1) == 1 ? a < b : a <= b;
  return (base != (bool)(c & 1u)) ? PV_TRUE : PV_FALSE;
}
// Unchanged on the successor: the changed node is not read, or the word holding each field read
// from it is the same in the old and the new node.
DSL_HD bool field_leaf_unchanged(const DevPred& pr, const NodeView& v) {
  if (!((pr.reads >> v.changed) & 1u)) return true;
  const uint32_t* old = v.base + v.changed * v.nw;
  const uint32_t l = (uint32_t)pr.arg0, r = (uint32_t)pr.arg1;
  uint32_t d = 0;
  if (DSL_FIELD_NODE(l) == v.changed) d |= old[DSL_FIELD_BIT(l) >> 5] ^ v.over[DSL_FIELD_BIT(l) >> 5];
  if ((pr.pad & kFieldRhsIsField) && DSL_FIELD_NODE(r) == v.changed)
    d |= old[DSL_FIELD_BIT(r) >> 5] ^ v.over[DSL_FIELD_BIT(r) >> 5];
  return d == 0;
}

// ---- the generic network leaf (DSL_PRED_NET, include/dslabs_hip.h) -------------------------------
// "network() holds a record satisfying all of the leaf's conditions", each an unsigned comparison
// of a bit field of the record with a constant; judged here for every protocol.
// Within one search the network only grows (delivery never removes a record, and the dropped
// records are constant), so the leaf can differ between a parent and its successor only through
// the successor's NEW records: when none of them matches, the leaf has the parent's value,
// whatever that was (also inside a program, where the parent's leaf value is unknown); when one
// matches it is true without a look at the parent.
template <class Rec>
DSL_HD bool rec_cond_holds(const DevRecCond c, Rec r) {
  uint32_t x;
  if constexpr (sizeof(Rec) == 8) x = (uint32_t)((uint64_t)r >> c.bit);  // may cross bit 32: shifted as one value
  else x = (uint32_t)r >> c.bit;
  if (c.width < 32) x &= (1u << c.width) - 1u;  // no 1u << 32
  // DSL_CMP_*: bits 1-2 pick ==, < or <=; bit 0 negates (NE, GE, GT)
  const bool base = (c.cmp >> 1) == 0 ? x == c.k : (c.cmp >> 1) == 1 ? x < c.k : x <= c.k;
  return base != (bool)(c.cmp & 1u);
}
template <class Rec>
DSL_HD bool rec_matches(const DevRecCond* conds, int n, Rec r) {
  bool ok = true;
  for (int i = 0; i < n; i++) ok &= rec_cond_holds<Rec>(conds[i], r);
  return ok;
}
// The hit mask (NodeView::net_hits) of a successor from its delta. Every access to the send list
// uses a compile-time index (the loop over the sends is innermost and fully unrolled, the
// conditions are read with wave-uniform indexes), so the records stay in VGPRs: no LDS staging,
// no scratch. `alive` bit q: kept send q has satisfied the leaf's conditions so far.
template <class P>
DSL_HD uint32_t delta_net_hits(const DevSettings& set, const Delta<P>& d) {
  uint32_t hits = 0;
  if (d.keep == 0u) return 0u;
  for (int i = 0; i < set.n_ops; i++) {
    const DevPred& op = set.ops[i];
    if (op.id != DSL_PRED_NET) continue;
    uint32_t alive = d.keep;
    for (int c = 0; c < op.arg1; c++) {
      const DevRecCond rc = set.rec_conds[op.arg0 + c];
#pragma unroll
      for (int q = 0; q < P::kMaxSends; q++)
        if (((alive >> q) & 1u) && !rec_cond_holds<typename P::Rec>(rc, d.out.r[q])) alive &= ~(1u << q);
    }
    if (alive) hits |= 1u << op.pad;
  }
  return hits;
}
// The same from a compacted list of the new records (host code).
template <class P>
inline uint32_t sends_net_hits(const DevSettings& set, const typename P::Rec* s, int n) {
  uint32_t hits = 0;
  for (int i = 0; i < set.n_ops; i++) {
    const DevPred& op = set.ops[i];
    if (op.id != DSL_PRED_NET) continue;
    for (int j = 0; j < n; j++)
      if (rec_matches<typename P::Rec>(set.rec_conds + op.arg0, op.arg1, s[j])) hits |= 1u << op.pad;
  }
  return hits;
}
// The same for the records a whole row holds and the dropped records (NodeView::row_hits): the
// scan of the parent's network(). The kernels run it where few registers are live (before the
// handler), and only when the judge will ask for it (net_needs_row): never on the common path,
// where a leaf is a whole predicate and the view is incremental.
template <class P>
DSL_HD uint32_t row_net_hits(const DevSettings& set, const uint32_t* w) {
  using Rec = typename P::Rec;
  uint32_t hits = 0;
  const int n = Net<P>::size(w);
  const Rec* x = static_cast<const Rec*>(set.dropped());
  for (int i = 0; i < set.n_ops; i++) {
    const DevPred& op = set.ops[i];
    if (op.id != DSL_PRED_NET) continue;
    bool m = false;
    for (int j = 0; j < n && !m; j++) m = rec_matches<Rec>(set.rec_conds + op.arg0, op.arg1, Net<P>::at(w, j));
    for (int j = 0; j < set.n_dropped && !m; j++) m = rec_matches<Rec>(set.rec_conds + op.arg0, op.arg1, x[j]);
    if (m) hits |= 1u << op.pad;
  }
  return hits;
}
// Whether judging a view needs row_hits: not when every program is one leaf and the view is
// incremental -- a network leaf is then either skipped (no new record matches: the parent's
// value) or true by its new records. Inside a program every leaf is evaluated once any leaf
// changed, a network leaf without a hit too, and a view that is not incremental evaluates all.
DSL_HD bool net_needs_row(const DevSettings& set, bool incremental, int changed) {
  return set.n_net != 0 && !(incremental && changed >= 0 && set.flat);
}
// ... and always when a watch (dsl_set_watches) holds a network leaf: a watch's value on the parent
// is unknown, so its leaf reads the new records, the parent's records and the dropped records. A
// function of its own, asked only where watches are counted (k_level<P, false, true>): the other
// callers of net_needs_row compile what they compiled before.
DSL_HD bool watch_needs_row(const DevSettings& set) { return set.watch_net != 0; }
// A new record matches, or one of the row's, or a dropped one.
DSL_HD int eval_net_leaf(const DevPred& pr, const NodeView& v) {
  return (((v.net_hits | v.row_hits) >> pr.pad) & 1u) ? PV_TRUE : PV_FALSE;
}
DSL_HD bool net_leaf_unchanged(const DevPred& pr, const NodeView& v) { return !((v.net_hits >> pr.pad) & 1u); }

// kField (here and below): the judge knows the generic leaves (the field leaf and the network leaf). Host code always does; a kernel is
// instantiated without it for the searches whose settings hold none (kernels.hpp: FIELD).
template <class P, bool kField = true>
DSL_HD bool leaf_unchanged(const DevPred& pr, const NodeView& v) {
  if constexpr (kField) {
    if (pr.id == DSL_PRED_FIELD) return field_leaf_unchanged(pr, v);
    if (pr.id == DSL_PRED_NET) return net_leaf_unchanged(pr, v);
  }
  if (pr.reads >> 31) return false;
  if (!((pr.reads >> v.changed) & 1u)) return true;
  return PredSame<P>::same(pr, v.base + v.changed * v.nw, v.over);
}
// A program is unchanged when every leaf is.
template <class P, bool kField = true>
DSL_HD bool prog_unchanged(const DevSettings& set, DevProg g, const NodeView& v, bool incremental) {
  if (!incremental || v.changed < 0) return false;
  for (int i = 0; i < g.len; i++) {
    const DevPred& op = set.ops[g.start + i];
    if (op.id > 0 && !leaf_unchanged<P, kField>(op, v)) return false;
  }
  return true;
}

// StatePredicate.test of a program (false / true / threw): postfix over a stack of 2-bit values
// kept in one word (no indexed private array). Combinators follow StatePredicate.java:397-431: a
// throwing left operand throws; and(a, b) is a when a is false, else b; or(a, b) is a when a is
// true, else b; negate keeps a throw.
template <class P, bool kField = true>
DSL_HD int eval_prog(const DevSettings& set, DevProg g, const NodeView& v, const typename P::Params& prm) {
  uint32_t st = 0;
  for (int i = 0; i < g.len; i++) {
    const DevPred& op = set.ops[g.start + i];
    int x;
    if (op.id == kOpAnd || op.id == kOpOr) {
      const int b = (int)(st & 3u);
      st >>= 2;
      const int a = (int)(st & 3u);
      st >>= 2;
      x = a == PV_THREW ? PV_THREW : op.id == kOpAnd ? (a == PV_FALSE ? PV_FALSE : b) : (a == PV_TRUE ? PV_TRUE : b);
    } else if (op.id == kOpNot) {
      const int a = (int)(st & 3u);
      st >>= 2;
      x = a == PV_THREW ? PV_THREW : !a;
    } else {
      if constexpr (kField) {
        x = op.id == DSL_PRED_FIELD ? eval_field_leaf(op, v)
            : op.id == DSL_PRED_NET ? eval_net_leaf(op, v)
                                    : P::eval(op, v, prm);
      } else {
        x = P::eval(op, v, prm);
      }
      if (x != PV_THREW && op.negate) x = !x;
    }
    st = (st << 2) | (uint32_t)x;
  }
  return (int)(st & 3u);
}

// A leaf known to hold on the parent (an invariant, not negated, of an expanded parent: the view is
// incremental) may be evaluated on the successor from what the changed node's words changed: a
// protocol may provide
//   static int eval_held(const DevPred&, const NodeView&, const Params&, bool held)
// (Multi-Paxos LOGS_CONSISTENT: only the slots whose entries the changed server changed, the other
// slots are as valid as on the parent); it must equal eval whenever held is true of the parent
// (tests/hostcheck compares the incremental verdict with the full one on every explored successor).
template <class P, class = void>
struct EvalHeld {
  static DSL_HD int eval(const DevPred& pr, const NodeView& v, const typename P::Params& prm, bool) {
    return P::eval(pr, v, prm);
  }
};
template <class P>
struct EvalHeld<P, std::void_t<decltype(&P::eval_held)>> {
  static DSL_HD int eval(const DevPred& pr, const NodeView& v, const typename P::Params& prm, bool held) {
    return P::eval_held(pr, v, prm, held);
  }
};

// checkState order over a node view (Search.java:162-231).
// incremental: the view is a successor of an EXPANDED, non-initial parent, which therefore had
// every invariant true, every goal false or throwing (ignored) and every prune false (a state
// that violated, matched or was pruned is never expanded; only the initial state is expanded
// when pruned, Search.java:475). A predicate whose leaves read neither the changed node's
// relevant words nor the network has the parent's value, so it is skipped with that outcome.
// tests/hostcheck checks the incremental verdict against the full one on every successor.
// The invariants, goals and prunes are walked as ONE sequence (programs [0, n_inv) are the
// invariants, then the goals, then the prunes), so the protocol's predicate code is inlined once
// rather than once per kind.
template <class P, bool kField = true>
DSL_HD Verdict judge_view(const NodeView& v0, const typename P::Params& prm, const DevSettings& set, int depth,
                          int* pred_index, bool incremental = false) {
  NodeView v = v0;
  if constexpr (NetPreds<P>::value) {
    v.dropped = set.dropped();
    v.ndropped = set.n_dropped;
  }
#ifndef __HIP_DEVICE_COMPILE__
  // host code hands over the new records as a list and leaves the row's scan to the judge (the
  // kernels computed both masks themselves: net_hits from registers, row_hits ahead of the handler)
  if (set.n_net) {
    if (v.sends) v.net_hits |= sends_net_hits<P>(set, static_cast<const typename P::Rec*>(v.sends), v.nsends);
    if (net_needs_row(set, incremental, v.changed)) v.row_hits = row_net_hits<P>(set, v.base);
  }
#endif
  const int ng = set.n_inv + set.n_goal, nt = ng + set.n_prune;
  if (set.flat) {
    // every program is one leaf (resolve_settings): program t IS ops[t], in checkState order
    // (invariants, goals, prunes) -- no program descriptors, no stack machine
    for (int t = 0; t < nt; t++) {
      const DevPred& op = set.ops[t];
      if (incremental && v.changed >= 0 && leaf_unchanged<P, kField>(op, v)) continue;
      int x;
      if constexpr (kField) {
        x = op.id == DSL_PRED_FIELD
                ? eval_field_leaf(op, v)
            : op.id == DSL_PRED_NET
                ? eval_net_leaf(op, v)
                : EvalHeld<P>::eval(op, v, prm, incremental && v.changed >= 0 && t < set.n_inv && !op.negate);
      } else {
        x = EvalHeld<P>::eval(op, v, prm, incremental && v.changed >= 0 && t < set.n_inv && !op.negate);
      }
      if (x != PV_THREW && op.negate) x = !x;
      if (t < set.n_inv) {
        if (x != PV_TRUE) {  // a false or throwing invariant is violated
          *pred_index = t;
          return V_TERM_INVARIANT;
        }
      } else if (t < ng) {
        if (x == PV_TRUE) {  // throwing goals are ignored
          *pred_index = t - set.n_inv;
          return V_TERM_GOAL;
        }
      } else if (x != PV_FALSE) {
        return V_PRUNED;  // true or throwing
      }
    }
    if (set.max_depth >= 0 && depth >= set.max_depth) return V_PRUNED;
    return V_VALID;
  }
  for (int t = 0; t < nt; t++) {
    const int kind = t < set.n_inv ? 0 : t < ng ? 1 : 2;
    const int i = kind == 0 ? t : kind == 1 ? t - set.n_inv : t - ng;
    const DevProg g = kind == 0 ? set.inv[i] : kind == 1 ? set.goal[i] : set.prune[i];
    if (prog_unchanged<P, kField>(set, g, v, incremental)) continue;
    const int x = eval_prog<P, kField>(set, g, v, prm);
    if (kind == 0 && x != PV_TRUE) {  // a false or throwing invariant is violated
      *pred_index = i;
      return V_TERM_INVARIANT;
    }
    if (kind == 1 && x == PV_TRUE) {  // throwing goals are ignored
      *pred_index = i;
      return V_TERM_GOAL;
    }
    if (kind == 2 && x != PV_FALSE) return V_PRUNED;  // true or throwing
  }
  if (set.max_depth >= 0 && depth >= set.max_depth) return V_PRUNED;
  return V_VALID;
}

// The watches (dsl_set_watches) of a view: bit w = watch w holds (true after its negation; a watch
// that throws does not hold). Evaluation is always full -- P::eval, eval_field_leaf, eval_net_leaf
// over net_hits | row_hits: the view's state is newly discovered, whatever its verdict, and no
// watch's value on its parent is known (a parent may hold a watch or not, unlike an invariant), so
// none of the judge's "keeps the parent's value" shortcuts applies (leaf_unchanged, EvalHeld).
// The kernel hands over both hit masks (row_hits computed ahead of the handler, net_needs_row with
// `watches`); host code gets them here, as in judge_view.
template <class P>
DSL_HD uint32_t eval_watches(const NodeView& v0, const typename P::Params& prm, const DevSettings& set) {
  NodeView v = v0;
  if constexpr (NetPreds<P>::value) {
    v.dropped = set.dropped();
    v.ndropped = set.n_dropped;
  }
#ifndef __HIP_DEVICE_COMPILE__
  if (set.n_net) {
    if (v.sends) v.net_hits |= sends_net_hits<P>(set, static_cast<const typename P::Rec*>(v.sends), v.nsends);
    v.row_hits = row_net_hits<P>(set, v.base);
  }
#endif
  uint32_t held = 0;
#pragma nounroll  // one copy of the predicate code; the trip count is wave-uniform
  for (int w = 0; w < set.n_watch; w++)
    if (eval_prog<P, true>(set, set.watch[w], v, prm) == PV_TRUE) held |= 1u << w;
  return held;
}

// Fills DevPred::reads of every leaf from the protocol's read sets (host, after resolve_settings).
// A field leaf reads exactly its node, or its two nodes (the protocol is not asked: it would
// answer kReadsAll for an id it does not know).
template <class P>
void set_pred_reads(DevSettings& d, const typename P::Params& prm) {
  for (int i = 0; i < d.n_ops; i++) {
    DevPred& op = d.ops[i];
    if (op.id == DSL_PRED_FIELD) {
      op.reads = 1u << DSL_FIELD_NODE((uint32_t)op.arg0);
      if (op.pad & kFieldRhsIsField) op.reads |= 1u << DSL_FIELD_NODE((uint32_t)op.arg1);
    } else if (op.id == DSL_PRED_NET) {
      op.reads = 1u << 31;  // the network only (its own incremental rule: net_leaf_unchanged)
    } else if (op.id > 0) {
      op.reads = P::pred_reads(op, prm);
    }
  }
}

// The one check of a field leaf that needs the protocol: the field lies inside the node's words
// (resolve_settings checked the rest). Host; false with the fault named in *why.
template <class P>
bool check_field_leaves(const DevSettings& d, std::string* why) {
  for (int i = 0; i < d.n_ops; i++) {
    const DevPred& op = d.ops[i];
    if (op.id != DSL_PRED_FIELD) continue;
    const uint32_t descs[2] = {(uint32_t)op.arg0, (uint32_t)op.arg1};
    for (int k = 0; k < ((op.pad & kFieldRhsIsField) ? 2 : 1); k++) {
      const int bit = DSL_FIELD_BIT(descs[k]), width = DSL_FIELD_WIDTH(descs[k]);
      if (bit + width > 32 * P::kNodeWords) {
        *why = std::string("field predicate: ") + (k ? "right" : "left") + " operand (node " +
               std::to_string(DSL_FIELD_NODE(descs[k])) + ", bit " + std::to_string(bit) + ", width " +
               std::to_string(width) + "): beyond the node's " + std::to_string(32 * P::kNodeWords) + " bits";
        return false;
      }
    }
  }
  return true;
}

// The same for a network leaf: every condition's field lies inside the record.
template <class P>
bool check_net_leaves(const DevSettings& d, std::string* why) {
  for (int i = 0; i < d.n_ops; i++) {
    const DevPred& op = d.ops[i];
    if (op.id != DSL_PRED_NET) continue;
    for (int c = 0; c < op.arg1; c++) {
      const DevRecCond& rc = d.rec_conds[op.arg0 + c];
      if (rc.bit + rc.width > 8 * (int)sizeof(typename P::Rec)) {
        *why = "network predicate: condition " + std::to_string(c) + " (bit " + std::to_string(rc.bit) + ", width " +
               std::to_string(rc.width) + "): beyond the record's " + std::to_string(8 * sizeof(typename P::Rec)) + " bits";
        return false;
      }
    }
  }
  return true;
}

// ---- step invariants (dsl_set_step_invariants, include/dslabs_hip.h) ------------------------------
// A step invariant is judged on an edge (P, E, X). The judge's delta view already holds both sides:
// v.base + i * v.nw is node i of P, v.node(i) node i of X. Functions of their own, shared by
// k_step_check and the host walk (tests/hostcheck/stepcheck.cpp): eval_prog, which every
// k_level<P, *, true> compiles, has no branch for them.
DSL_HD uint32_t step_field_read(const NodeView& v, uint32_t desc, bool from_new) {
  const int bit = DSL_FIELD_BIT(desc), width = DSL_FIELD_WIDTH(desc), node = DSL_FIELD_NODE(desc);
  const uint32_t* w = from_new ? v.node(node) : v.base + node * v.nw;
  const uint32_t x = w[bit >> 5] >> (bit & 31);
  return width >= 32 ? x : x & ((1u << width) - 1u);  // no 1u << 32
}
DSL_HD int eval_step_field_leaf(const DevPred& pr, const NodeView& v) {
  const uint32_t a = step_field_read(v, (uint32_t)pr.arg0, (pr.pad & kStepLhsNew) != 0u);
  const uint32_t b = (pr.pad & kFieldRhsIsField) ? step_field_read(v, (uint32_t)pr.arg1, (pr.pad & kStepRhsNew) != 0u)
                                                 : (uint32_t)pr.arg1;
  const uint32_t c = pr.pad & 7u;  // DSL_CMP_*, as eval_field_leaf
  const bool base = (c >> 1) == 0 ? a == b : (c >> 1) == 1 ? a < b : a <= b;
  return (base != (bool)(c & 1u)) ? PV_TRUE : PV_FALSE;
}
// The step hit mask of an edge from its delta: bit i = a KEPT send (a record new to the parent's
// set) satisfies DSL_PRED_STEP_SENT leaf i (DevPred::pad). Over the step ops only; the send list is
// read through compile-time indices, as delta_net_hits reads it.
template <class P>
DSL_HD uint32_t delta_step_hits(const DevSettings& set, const DevStep& step, const Delta<P>& d) {
  uint32_t hits = 0;
  if (d.keep == 0u || step.n_sent == 0) return 0u;
  for (int i = step.op0; i < step.op1; i++) {
    const DevPred& op = set.ops[i];
    if (op.id != DSL_PRED_STEP_SENT) continue;
    uint32_t alive = d.keep;
    for (int c = 0; c < op.arg1; c++) {
      const DevRecCond rc = set.rec_conds[op.arg0 + c];
#pragma unroll
      for (int q = 0; q < P::kMaxSends; q++)
        if (((alive >> q) & 1u) && !rec_cond_holds<typename P::Rec>(rc, d.out.r[q])) alive &= ~(1u << q);
    }
    if (alive) hits |= 1u << op.pad;
  }
  return hits;
}
// StatePredicate.test of a step program on the edge whose successor `v` views: eval_prog's stack
// machine and three-valued rules with the step leaves added. hits: delta_step_hits; cls / to: the
// event's handler class and node (read only by a DSL_PRED_STEP_EVENT leaf). DSL_PRED_FIELD and the
// protocol's named leaves are evaluated on the successor.
template <class P>
DSL_HD int eval_step_prog(const DevSettings& set, DevProg g, const NodeView& v0, const typename P::Params& prm,
                          uint32_t hits, int cls, int to) {
  NodeView v = v0;
  if constexpr (NetPreds<P>::value) {  // the successor's network() includes the dropped set, as in judge_view
    v.dropped = set.dropped();
    v.ndropped = set.n_dropped;
  }
  uint32_t st = 0;
  for (int i = 0; i < g.len; i++) {
    const DevPred& op = set.ops[g.start + i];
    int x;
    if (op.id == kOpAnd || op.id == kOpOr) {
      const int b = (int)(st & 3u);
      st >>= 2;
      const int a = (int)(st & 3u);
      st >>= 2;
      x = a == PV_THREW ? PV_THREW : op.id == kOpAnd ? (a == PV_FALSE ? PV_FALSE : b) : (a == PV_TRUE ? PV_TRUE : b);
    } else if (op.id == kOpNot) {
      const int a = (int)(st & 3u);
      st >>= 2;
      x = a == PV_THREW ? PV_THREW : !a;
    } else {
      x = op.id == DSL_PRED_STEP_FIELD   ? eval_step_field_leaf(op, v)
          : op.id == DSL_PRED_STEP_SENT  ? (((hits >> op.pad) & 1u) ? PV_TRUE : PV_FALSE)
          : op.id == DSL_PRED_STEP_EVENT ? (((op.arg0 < 0 || op.arg0 == cls) && (op.arg1 < 0 || op.arg1 == to)) ? PV_TRUE : PV_FALSE)
          : op.id == DSL_PRED_FIELD      ? eval_field_leaf(op, v)
                                         : P::eval(op, v, prm);
      if (x != PV_THREW && op.negate) x = !x;
    }
    st = (st << 2) | (uint32_t)x;
  }
  return (int)(st & 3u);
}
// The handler class and node of located event e of parent row w, as the event census classifies it
// (an event the no-op filters would skip has its real class).
template <class P>
DSL_HD void step_event_cell(const uint32_t* w, int e, const typename P::Params& prm, int* cls, int* to) {
  if (e >= 0) {
    const auto r = Net<P>::at(w, e);
    *cls = P::msg_class(r);
    *to = P::rec_to(r);
  } else {
    *to = (-1 - e) >> 8;
    *cls = Classes<P>::kTimer0 + TimerClasses<P>::of(*to, prm);
  }
}
// The checks of the step ops that need the protocol (resolve_settings made the rest; the loops of
// check_field_leaves / check_net_leaves / set_pred_reads end at n_ops and never see a step op):
// fields inside the node, conditions inside the record, the class among the protocol's; the read
// set of a named leaf, which its P::eval may consult.
template <class P>
bool check_step_leaves(DevSettings& d, const DevStep& step, const typename P::Params& prm, std::string* why) {
  for (int i = step.op0; i < step.op1; i++) {
    DevPred& op = d.ops[i];
    if (op.id == DSL_PRED_FIELD || op.id == DSL_PRED_STEP_FIELD) {
      const uint32_t descs[2] = {(uint32_t)op.arg0, (uint32_t)op.arg1};
      for (int k = 0; k < ((op.pad & kFieldRhsIsField) ? 2 : 1); k++) {
        const int bit = DSL_FIELD_BIT(descs[k]), width = DSL_FIELD_WIDTH(descs[k]);
        if (bit + width > 32 * P::kNodeWords) {
          *why = std::string("field predicate: ") + (k ? "right" : "left") + " operand (node " +
                 std::to_string(DSL_FIELD_NODE(descs[k])) + ", bit " + std::to_string(bit) + ", width " +
                 std::to_string(width) + "): beyond the node's " + std::to_string(32 * P::kNodeWords) + " bits";
          return false;
        }
      }
    } else if (op.id == DSL_PRED_STEP_SENT) {
      for (int c = 0; c < op.arg1; c++) {
        const DevRecCond& rc = d.rec_conds[op.arg0 + c];
        if (rc.bit + rc.width > 8 * (int)sizeof(typename P::Rec)) {
          *why = "network predicate: condition " + std::to_string(c) + " (bit " + std::to_string(rc.bit) + ", width " +
                 std::to_string(rc.width) + "): beyond the record's " + std::to_string(8 * sizeof(typename P::Rec)) + " bits";
          return false;
        }
      }
    } else if (op.id == DSL_PRED_STEP_EVENT) {
      if (op.arg0 >= Classes<P>::kSkip) {
        *why = "step event leaf: class " + std::to_string(op.arg0) + " outside the protocol's " +
               std::to_string((int)Classes<P>::kSkip) + " handler classes";
        return false;
      }
    } else if (op.id > 0) {
      op.reads = P::pred_reads(op, prm);
    }
  }
  return true;
}

}  // namespace dsl
