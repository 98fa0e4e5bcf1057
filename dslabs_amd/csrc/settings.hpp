// settings.hpp -- dsl_settings (TestSettings + SearchSettings) -> DevSettings, host side.
// Shared by the engine (engine.hip) and the host-only CPU baseline (tools/cpu_bfs.cpp).
#pragma once
#include <functional>
#include <string>

#include "common.hpp"

namespace dsl {

// TestSettings.shouldDeliver precedence (TestSettings.java:224-245): self-send always; then
// link override, sender override, receiver override, global networkActive.
// TestSettings.deliverTimers(a): per-address override else the global flag (:87-89).
// watches (optional): compiled behind the settings' own predicates into the same ops[] and
// rec_conds[], with the same checks; a failure leaves *out untouched.
inline int resolve_settings(const dsl_settings& in, int num_nodes, bool (*known)(int), DevSettings* out,
                            std::string* why_out, const WatchList* watches = nullptr) {
  DevSettings d{};
  if (num_nodes > DSL_MAX_NODES) return *why_out = "too many nodes", DSL_ERR_ARG;
  if (in.do_checks < DSL_CHECKS_NONE || in.do_checks > DSL_CHECKS_ALL || in.check_sample < 0)
    return *why_out = "do_checks must be DSL_CHECKS_NONE / _ERRORS / _ALL and check_sample >= 0", DSL_ERR_ARG;
  for (int f = 0; f < num_nodes; f++) {
    uint32_t row = 0;
    for (int t = 0; t < num_nodes; t++) {
      bool ok;
      if (f == t) ok = true;
      else if (in.link_active[f][t] >= 0) ok = in.link_active[f][t] != 0;
      else if (in.sender_active[f] >= 0) ok = in.sender_active[f] != 0;
      else if (in.receiver_active[t] >= 0) ok = in.receiver_active[t] != 0;
      else ok = in.network_active != 0;
      if (ok) row |= 1u << t;
    }
    d.deliver[f] = row;
  }
  d.all_deliver = 1;
  for (int f = 0; f < num_nodes; f++)
    if ((d.deliver[f] & ((num_nodes >= 32 ? 0u : (1u << num_nodes)) - 1u)) != ((num_nodes >= 32 ? 0u : (1u << num_nodes)) - 1u))
      d.all_deliver = 0;
  for (int a = 0; a < num_nodes; a++) {
    bool ok = in.timers_active[a] >= 0 ? in.timers_active[a] != 0 : in.deliver_timers != 0;
    if (ok) d.timer_mask |= 1u << a;
  }
  d.max_depth = in.max_depth;
  if (in.n_invariants < 0 || in.n_invariants > DSL_MAX_PREDICATES || in.n_goals < 0 ||
      in.n_goals > DSL_MAX_PREDICATES || in.n_prunes < 0 || in.n_prunes > DSL_MAX_PREDICATES || in.n_pool < 0 ||
      in.n_pool > DSL_MAX_POOL)
    return *why_out = "predicate counts out of range", DSL_ERR_ARG;
  d.n_inv = in.n_invariants;
  d.n_goal = in.n_goals;
  d.n_prune = in.n_prunes;
  // predicate trees (leaves + DSL_PRED_AND / _OR / _IMPLIES over pool entries) -> postfix programs
  std::string why;
  int n_rec = 0;  // entries of d.rec_conds in use
  const dsl_predicate* pool = in.pool;  // the operands of what is being compiled (the watches bring their own)
  int n_pool = in.n_pool;
  std::function<bool(const dsl_predicate&, int, int*)> emit = [&](const dsl_predicate& p, int level, int* sp) -> bool {
    if (level > 16) return why = "predicate nesting too deep", false;
    const bool comb = p.pred_id == DSL_PRED_AND || p.pred_id == DSL_PRED_OR || p.pred_id == DSL_PRED_IMPLIES;
    if (comb) {
      if (p.arg0 < 0 || p.arg0 >= n_pool || p.arg1 < 0 || p.arg1 >= n_pool)
        return why = "combinator operand outside dsl_settings.pool", false;
      if (!emit(pool[p.arg0], level + 1, sp)) return false;
      auto push_op = [&](int32_t op) {
        if (d.n_ops >= kMaxProgOps) return why = "predicate programs too long", false;
        d.ops[d.n_ops++] = DevPred{op, 0, 0, 0, 0u, 0u};
        return true;
      };
      if (p.pred_id == DSL_PRED_IMPLIES && !push_op(kOpNot)) return false;  // or(negate(a), b)
      if (!emit(pool[p.arg1], level + 1, sp)) return false;
      if (!push_op(p.pred_id == DSL_PRED_AND ? kOpAnd : kOpOr)) return false;
      (*sp)--;
      if (p.negate && !push_op(kOpNot)) return false;
      return true;
    }
    if (p.pred_id == DSL_PRED_FIELD) {
      // the generic field leaf: every protocol's (the judge evaluates it, not P::eval); packed
      // into the DevPred's 96 argument bits. The one check that needs the protocol's words per
      // node is check_field_leaves<P> (nodestate.hpp), where P is known.
      const uint64_t a0 = (uint64_t)p.arg0, a1 = (uint64_t)p.arg1;
      const int cmp = DSL_FIELD_ARG0_CMP(a0), rhs_field = DSL_FIELD_ARG0_RHS_IS_FIELD(a0);
      if (a0 >> 36) return why = "field predicate: arg0 has bits set above the descriptor, comparison and operand kind", false;
      if (cmp > DSL_CMP_GT) return why = "field predicate: unknown comparison " + std::to_string(cmp), false;
      if (a1 >> 32) return why = "field predicate: arg1 does not fit in 32 unsigned bits", false;
      auto bad_desc = [&](uint32_t desc, const char* side) {
        const int node = DSL_FIELD_NODE(desc), bit = DSL_FIELD_BIT(desc), width = DSL_FIELD_WIDTH(desc);
        const std::string at = std::string("field predicate: ") + side + " operand (node " + std::to_string(node) +
                               ", bit " + std::to_string(bit) + ", width " + std::to_string(width) + "): ";
        if (desc & ~DSL_FIELD_DESC_MASK) return why = at + "descriptor has bits set above bit 26", true;
        if (node >= num_nodes) return why = at + "node index >= the protocol's " + std::to_string(num_nodes) + " nodes", true;
        if (width < 1 || width > 32) return why = at + "width outside 1..32", true;
        if ((bit & 31) + width > 32) return why = at + "field straddles a 32-bit word", true;
        return false;
      };
      if (bad_desc(DSL_FIELD_ARG0_DESC(a0), "left")) return false;
      if (rhs_field && bad_desc((uint32_t)a1, "right")) return false;
      if (d.n_ops >= kMaxProgOps) return why = "predicate programs too long", false;
      d.ops[d.n_ops++] = DevPred{p.pred_id, p.negate, (int32_t)DSL_FIELD_ARG0_DESC(a0), (int32_t)(uint32_t)a1, 0u,
                                 (uint32_t)cmp | (rhs_field ? kFieldRhsIsField : 0u)};
      if (++*sp > kMaxProgStack) return why = "predicate too wide", false;
      return true;
    }
    if (p.pred_id == DSL_PRED_NET) {
      // the generic network leaf: every protocol's. Its conditions (consecutive DSL_PRED_REC_COND
      // pool entries) go into DevSettings::rec_conds; the DevPred keeps (first, count) and the
      // leaf's ordinal. bit + width against the record's size is check_net_leaves<P>'s.
      if (p.arg1 < 1 || p.arg1 > DSL_MAX_NET_CONDS)
        return why = "network predicate: " + std::to_string(p.arg1) + " conditions, outside 1.." +
                     std::to_string(DSL_MAX_NET_CONDS), false;
      if (p.arg0 < 0 || p.arg0 > n_pool || p.arg0 + p.arg1 > n_pool)
        return why = "network predicate: condition range outside dsl_settings.pool", false;
      if (n_rec + (int)p.arg1 > kMaxRecConds)
        return why = "network predicate: more than " + std::to_string(kMaxRecConds) + " conditions in all", false;
      const int first = n_rec;
      for (int c = 0; c < (int)p.arg1; c++) {
        const dsl_predicate& q = pool[p.arg0 + c];
        const std::string at = "network predicate: condition " + std::to_string(c) + " (pool " + std::to_string(p.arg0 + c) + "): ";
        if (q.pred_id != DSL_PRED_REC_COND) return why = at + "not a DSL_PRED_REC_COND", false;
        const uint64_t a0 = (uint64_t)q.arg0, a1 = (uint64_t)q.arg1;
        const int width = DSL_REC_ARG0_WIDTH(a0), cmp = DSL_REC_ARG0_CMP(a0);
        if (q.negate) return why = at + "negate set on a record condition", false;
        if (a0 & ~DSL_REC_ARG0_MASK) return why = at + "arg0 has bits set outside bit, width and comparison", false;
        if (cmp > DSL_CMP_GT) return why = at + "unknown comparison " + std::to_string(cmp), false;
        if (width < 1 || width > 32) return why = at + "width outside 1..32", false;
        if (a1 >> 32) return why = at + "arg1 does not fit in 32 unsigned bits", false;
        d.rec_conds[n_rec++] = DevRecCond{(uint16_t)DSL_REC_ARG0_BIT(a0), (uint8_t)width, (uint8_t)cmp, (uint32_t)a1};
      }
      if (d.n_ops >= kMaxProgOps) return why = "predicate programs too long", false;
      d.ops[d.n_ops++] = DevPred{p.pred_id, p.negate, first, (int32_t)p.arg1, 0u, (uint32_t)d.n_net++};
      if (++*sp > kMaxProgStack) return why = "predicate too wide", false;
      return true;
    }
    if (p.pred_id == DSL_PRED_REC_COND)
      return why = "record condition (DSL_PRED_REC_COND) used as a predicate or a combinator operand: "
                   "it is legal only as a condition of a DSL_PRED_NET", false;
    if (!known(p.pred_id)) return why = "predicate not supported by this protocol's device predicates", false;
    if (d.n_ops >= kMaxProgOps) return why = "predicate programs too long", false;
    d.ops[d.n_ops++] = DevPred{p.pred_id, p.negate, (int32_t)p.arg0, (int32_t)p.arg1, 0u, 0u};
    if (++*sp > kMaxProgStack) return why = "predicate too wide", false;
    return true;
  };
  auto compile = [&](const dsl_predicate* src, int n, DevProg* dst) {
    for (int i = 0; i < n; i++) {
      const int start = d.n_ops;
      int sp = 0;
      if (!emit(src[i], 0, &sp)) return false;
      dst[i] = DevProg{(int16_t)start, (int16_t)(d.n_ops - start)};
    }
    return true;
  };
  if (!compile(in.invariants, d.n_inv, d.inv) || !compile(in.goals, d.n_goal, d.goal) ||
      !compile(in.prunes, d.n_prune, d.prune)) {
    *why_out = why;
    return why.rfind("predicate not supported", 0) == 0 ? DSL_ERR_UNKNOWN_PREDICATE : DSL_ERR_ARG;
  }
  d.flat = d.n_ops == d.n_inv + d.n_goal + d.n_prune ? 1 : 0;  // one leaf per program
  if (watches && watches->n != 0) {
    // behind the three lists (d.flat is theirs alone: a watch tree never switches the flat judge
    // off); network leaves of watches take the next ordinals of n_net
    if (watches->n < 0 || watches->n > DSL_MAX_WATCHES)
      return *why_out = "watches: " + std::to_string(watches->n) + ", outside 0.." + std::to_string(DSL_MAX_WATCHES), DSL_ERR_ARG;
    if (!watches->watches || watches->n_pool < 0 || watches->n_pool > DSL_MAX_POOL || (watches->n_pool > 0 && !watches->pool))
      return *why_out = "watches: predicate counts out of range", DSL_ERR_ARG;
    pool = watches->pool;
    n_pool = watches->n_pool;
    const int net0 = d.n_net;
    if (!compile(watches->watches, watches->n, d.watch)) {
      *why_out = why;
      return why.rfind("predicate not supported", 0) == 0 ? DSL_ERR_UNKNOWN_PREDICATE : DSL_ERR_ARG;
    }
    d.n_watch = watches->n;
    d.watch_net = d.n_net > net0 ? 1 : 0;
  }
  *out = d;
  return DSL_OK;
}

}  // namespace dsl
