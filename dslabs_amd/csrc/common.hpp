// common.hpp -- shared device/host types of the MI355X BFS engine.
//
// Every protocol is a struct with static __host__ __device__ transition functions over a
// fixed-width packed State (uint32 words). The engine (engine.hip) is templated on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dslabs_hip.h"

#define DSL_HD __host__ __device__ __forceinline__

namespace dsl {

// Outcome of applying the k-th enabled event to a state.
enum StepRc : int {
  STEP_OK = 0,
  STEP_NULL = 1,       // destination node missing (SearchState.stepMessage returns null)
  STEP_EXCEPTION = 2,  // handler "threw": exceptional, terminal, never equal to another state
  STEP_OVERFLOW = 3    // bounded container exceeded: hard engine error, never truncated
};

// Predicate value (StatePredicate.test): false / true / threw.
enum PredVal : int { PV_FALSE = 0, PV_TRUE = 1, PV_THREW = 2 };

// One step of a predicate program: a leaf (a standard or protocol predicate, optionally
// negated) or a combinator over the values on the program's stack (StatePredicate.and / or /
// implies / negate, T/StatePredicate.java:382-432). Programs are postfix; resolve_settings
// compiles the C ABI's predicate trees into them.
struct DevPred {
  int32_t id;      // leaf: dsl_predicate_id (> 0); combinator: kOpAnd / kOpOr / kOpNot
  int32_t negate;  // leaf: StatePredicate.negate()
  int32_t arg0, arg1;
  uint32_t reads;  // leaf: nodes whose words it reads (bit i = node i; bit 31 = the network)
  uint32_t pad;    // DSL_PRED_FIELD: DSL_CMP_* | kFieldRhsIsField (arg0 = the left field descriptor,
                   // arg1 = the constant or the right field descriptor, as bit patterns);
                   // DSL_PRED_NET: the leaf's ordinal among the settings' network leaves (its bit in
                   // NodeView::net_hits; arg0 = its first DevSettings::rec_conds entry, arg1 = how
                   // many); else 0
};
// One condition of a network leaf (DSL_PRED_REC_COND): (record >> bit) & mask(width) <cmp> k.
struct DevRecCond {
  uint16_t bit;
  uint8_t width;  // 1..32
  uint8_t cmp;    // DSL_CMP_*
  uint32_t k;
};
constexpr int kMaxRecConds = DSL_MAX_NET_CONDS_TOTAL;
constexpr int32_t kOpAnd = -1, kOpOr = -2, kOpNot = -3;
constexpr uint32_t kFieldRhsIsField = 8u;
constexpr uint32_t kReadsAll = 0xffffffffu;
constexpr int kMaxProgOps = 64;   // ops of all the programs of one search
constexpr int kMaxProgStack = 16;  // values on a program's stack (2 bits each in one word)

// A top-level predicate (an invariant, goal or prune): ops [start, start + len) of the pool.
struct DevProg {
  int16_t start, len;
};

// The engine's watches (dsl_set_watches): top-level predicates with a pool of their own.
struct WatchList {
  const dsl_predicate* watches = nullptr;
  int32_t n = 0;
  const dsl_predicate* pool = nullptr;
  int32_t n_pool = 0;
};

// The engine's step invariants (dsl_set_step_invariants): top-level predicates over an edge, with a
// pool of their own.
struct StepList {
  const dsl_predicate* preds = nullptr;
  int32_t n = 0;
  const dsl_predicate* pool = nullptr;
  int32_t n_pool = 0;
};
// DevPred::pad of a DSL_PRED_STEP_FIELD: DSL_CMP_* | kFieldRhsIsField | which side is read from the
// successor (else from the parent)
constexpr uint32_t kStepLhsNew = 16u, kStepRhsNew = 32u;
// Device form of the step invariants: programs over ops [op0, op1) of DevSettings::ops, BEHIND
// DevSettings::n_ops (no loop over ops[0, n_ops) sees a step op), their record conditions behind
// the watches' in DevSettings::rec_conds. k_step_check alone takes it, in its own argument struct:
// DevSettings keeps its layout and every other kernel its arguments.
struct DevStep {
  int32_t n_step = 0;
  int32_t op0 = 0, op1 = 0;
  int32_t n_sent = 0;     // DSL_PRED_STEP_SENT leaves; each has a bit of the step hit mask (DevPred::pad)
  int32_t has_event = 0;  // some leaf is a DSL_PRED_STEP_EVENT: the event's class and node are needed
  int32_t pad[3] = {0, 0, 0};
  DevProg prog[DSL_MAX_STEP_INVARIANTS] = {};
};

// Device form of SearchSettings/TestSettings. The tri-state precedence of
// TestSettings.shouldDeliver (TestSettings.java:224-245) is resolved on the host into a
// boolean matrix deliver[from] bit `to`; timers into timer_mask bit a = deliverTimers(a).
struct DevSettings {
  uint32_t deliver[DSL_MAX_NODES];
  uint32_t timer_mask;
  int32_t all_deliver;  // every (from, to) pair of the protocol's nodes delivers
  int32_t max_depth;
  int32_t n_inv, n_goal, n_prune, n_ops;
  // 1: every program is a single leaf (no combinator), so ops[t] is program t in checkState order
  // -- invariants, goals, prunes (resolve_settings emits them in that order); judge_view then walks
  // the leaves directly (no program descriptors, no stack)
  int32_t flat;
  int32_t n_net;  // network leaves (DSL_PRED_NET) among ops[]; each has a bit of NodeView::net_hits
  DevProg inv[DSL_MAX_PREDICATES];
  DevProg goal[DSL_MAX_PREDICATES];
  DevProg prune[DSL_MAX_PREDICATES];
  DevPred ops[kMaxProgOps];
  // SearchState.droppedNetwork (dsl_set_dropped): the records network predicates see beside the
  // state's own (network() = network + droppedNetwork, SearchState.java:153-157); the same
  // records in device memory (kernels) and host memory (host-side judging), P::Rec-typed.
  const void* dropped_dev;
  const void* dropped_host;
  int32_t n_dropped;
  int32_t pad_dropped;
  DSL_HD const void* dropped() const {
#ifdef __HIP_DEVICE_COMPILE__
    return dropped_dev;
#else
    return dropped_host;
#endif
  }
  // the conditions of the network leaves (behind everything else: the offsets of the fields the
  // kernels without the leaf read are what they were)
  DevRecCond rec_conds[kMaxRecConds];
  // the watches (dsl_set_watches): predicates that are only counted, programs over the same ops[]
  // behind those of the invariants, goals and prunes. Behind rec_conds for the same reason; only
  // k_level<P, false, true> reads them. watch_net: a watch holds a network leaf (its value on the
  // parent is unknown, so the judge needs the parent row's records: net_needs_row)
  int32_t n_watch;
  int32_t watch_net;
  DevProg watch[DSL_MAX_WATCHES];
  // the watches that want a witness and have none yet (dsl_set_watch_witnesses; bit w = watch w):
  // the level queue stops after a level that counted one of them (watch_wanted_hit), and
  // k_watch_witness selects among them. Behind everything else, as the watches are; the engine
  // sets it per launch (BfsEngine::seed_search, account_level), resolve_settings leaves it 0.
  uint32_t watch_want;
  uint32_t pad_watch;
};

// True when no active lane of the wavefront has `p` (device; one thread on the host): the exit of
// a fixed-trip loop over a per-lane list once every lane is past its end (the unrolled iterations
// after it would each still pay their exec-mask test and branch).
DSL_HD bool wave_none(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(p) == 0ull;
#else
  return !p;
#endif
}

DSL_HD bool should_deliver(const DevSettings& s, int from, int to) {
  return (s.deliver[from] >> to) & 1u;
}
DSL_HD bool deliver_timers(const DevSettings& s, int a) { return (s.timer_mask >> a) & 1u; }

// Bit-field access into a packed state. Fields never straddle a 32-bit word.
template <int W>
struct Packed {
  uint32_t w[W];
  DSL_HD uint32_t get(int bitoff, int width) const {
    return (w[bitoff >> 5] >> (bitoff & 31)) & ((width == 32) ? 0xffffffffu : ((1u << width) - 1u));
  }
  DSL_HD void set(int bitoff, int width, uint32_t v) {
    uint32_t m = ((width == 32) ? 0xffffffffu : ((1u << width) - 1u)) << (bitoff & 31);
    uint32_t& x = w[bitoff >> 5];
    x = (x & ~m) | ((v << (bitoff & 31)) & m);
  }
  DSL_HD bool bit(int b) const { return (w[b >> 5] >> (b & 31)) & 1u; }
  DSL_HD void setbit(int b) { w[b >> 5] |= 1u << (b & 31); }
};

// Word i of a node's N words for a run-time i: a select chain, so a node held in a per-lane
// array stays in VGPRs (a dynamically indexed private array is placed in scratch, and every
// handler access would then be a memory round trip). A constant i folds to one access.
template <int N>
DSL_HD uint32_t sel_word(const uint32_t* w, int i) {
  uint32_t v = w[0];
#pragma unroll
  for (int k = 1; k < N; k++) {
    uint32_t x = w[k];
#ifdef __HIP_DEVICE_COMPILE__
    // keeps the selection on VALUES: otherwise the optimizer folds the chain into one load
    // from a selected address, i.e. back into a dynamically indexed (scratch) array
    asm("" : "+v"(x));
#endif
    v = (i == k) ? x : v;
  }
  return v;
}
template <int N>
DSL_HD void sel_put(uint32_t* w, int i, uint32_t v) {
#pragma unroll
  for (int k = 0; k < N; k++) w[k] = (i == k) ? v : w[k];
}
// An opaque copy of v: per-element selects over a private array stay selects of VALUES (the
// optimizer would otherwise merge them into one access at a computed address, and a dynamically
// addressed private array -- or a kernel-argument struct -- is copied to scratch memory).
template <class T>
DSL_HD T keep_value(T v) {
#ifdef __HIP_DEVICE_COMPILE__
  asm("" : "+v"(v));
#endif
  return v;
}
// a[r][c] of a small parameter table for run-time r, c (a select chain, see keep_value).
template <int R, int C>
DSL_HD int sel_param(const int32_t (&a)[R][C], int r, int c) {
  int v = 0;
#pragma unroll
  for (int i = 0; i < R; i++)
#pragma unroll
    for (int j = 0; j < C; j++) v = (i == r && j == c) ? keep_value((int)a[i][j]) : v;
  return v;
}

// Bit-field get/put over a node's N words (fields never straddle a word).
template <int N>
DSL_HD int field_get(const uint32_t* w, int bit, int width) {
  return (int)((sel_word<N>(w, bit >> 5) >> (bit & 31)) & ((1u << width) - 1u));
}
template <int N>
DSL_HD void field_put(uint32_t* w, int bit, int width, int v) {
  const uint32_t m = ((1u << width) - 1u) << (bit & 31);
  const int i = bit >> 5;
  sel_put<N>(w, i, (sel_word<N>(w, i) & ~m) | (((uint32_t)v << (bit & 31)) & m));
}

// How a successor is judged (Search.checkState, Search.java:162-231).
enum Verdict : int { V_VALID = 0, V_PRUNED = 1, V_TERM_EXCEPTION = 2, V_TERM_INVARIANT = 3, V_TERM_GOAL = 4 };

}  // namespace dsl
