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
// steps (optional, with step_out): the step invariants (dsl_set_step_invariants), compiled after
// everything else into ops[n_ops, ...) and rec_conds behind the watches' -- n_ops, n_net, flat,
// watch_net and the read sets are what they are without them, so no loop over ops[0, n_ops) ever
// sees a step op -- and described in *step_out. A failure leaves *out and *step_out untouched.
inline int resolve_settings(const dsl_settings& in, int num_nodes, bool (*known)(int), DevSettings* out,
                            std::string* why_out, const WatchList* watches = nullptr, const StepList* steps = nullptr,
                            DevStep* step_out = nullptr) {
  DevSettings d{};
  DevStep ds{};
  bool in_step = false;              // compiling a step invariant: the step leaves are legal, DSL_PRED_NET is not
  const char* list_name = "invariants";  // the list being compiled, for the refusals' text
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
    if (p.pred_id == DSL_PRED_STEP_FIELD || p.pred_id == DSL_PRED_STEP_SENT || p.pred_id == DSL_PRED_STEP_EVENT) {
      const char* leaf = p.pred_id == DSL_PRED_STEP_FIELD ? "DSL_PRED_STEP_FIELD"
                         : p.pred_id == DSL_PRED_STEP_SENT ? "DSL_PRED_STEP_SENT" : "DSL_PRED_STEP_EVENT";
      if (!in_step)
        return why = std::string("step leaf ") + leaf + " in the " + list_name +
                     ": a step leaf is legal only in a step invariant (dsl_set_step_invariants)", false;
    }
    if (in_step && p.pred_id == DSL_PRED_NET)
      return why = "DSL_PRED_NET in a step invariant is not supported: use DSL_PRED_STEP_SENT for the records the "
                   "step added", false;
    if (p.pred_id == DSL_PRED_STEP_EVENT) {
      // the class is checked against the protocol's classes in check_step_leaves<P>
      if (p.arg0 < -1 || p.arg0 > 15) return why = "step event leaf: class " + std::to_string(p.arg0) + " out of range", false;
      if (p.arg1 < -1 || p.arg1 >= num_nodes)
        return why = "step event leaf: node " + std::to_string(p.arg1) + " outside -1.." + std::to_string(num_nodes - 1), false;
      if (d.n_ops >= kMaxProgOps) return why = "predicate programs too long", false;
      d.ops[d.n_ops++] = DevPred{p.pred_id, p.negate, (int32_t)p.arg0, (int32_t)p.arg1, 0u, 0u};
      ds.has_event = 1;
      if (++*sp > kMaxProgStack) return why = "predicate too wide", false;
      return true;
    }
    if (p.pred_id == DSL_PRED_FIELD || p.pred_id == DSL_PRED_STEP_FIELD) {
      // the generic field leaf: every protocol's (the judge evaluates it, not P::eval); packed
      // into the DevPred's 96 argument bits. The one check that needs the protocol's words per
      // node is check_field_leaves<P> (nodestate.hpp), where P is known.
      const uint64_t a0 = (uint64_t)p.arg0, a1 = (uint64_t)p.arg1;
      const int cmp = DSL_FIELD_ARG0_CMP(a0), rhs_field = DSL_FIELD_ARG0_RHS_IS_FIELD(a0);
      const bool stepf = p.pred_id == DSL_PRED_STEP_FIELD;
      if (a0 >> (stepf ? 38 : 36))
        return why = "field predicate: arg0 has bits set above the descriptor, comparison and operand kind", false;
      if (stepf && DSL_STEP_ARG0_RHS_NEW(a0) && !rhs_field)
        return why = "field predicate: arg0 bit 37 (right operand from the successor) without a right field", false;
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
                                 (uint32_t)cmp | (rhs_field ? kFieldRhsIsField : 0u) |
                                     (stepf && DSL_STEP_ARG0_LHS_NEW(a0) ? kStepLhsNew : 0u) |
                                     (stepf && DSL_STEP_ARG0_RHS_NEW(a0) ? kStepRhsNew : 0u)};
      if (++*sp > kMaxProgStack) return why = "predicate too wide", false;
      return true;
    }
    if (p.pred_id == DSL_PRED_NET || p.pred_id == DSL_PRED_STEP_SENT) {
      // (DSL_PRED_STEP_SENT: the same pool encoding; its ordinal is among the step leaves, ds.n_sent)
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
      d.ops[d.n_ops++] = DevPred{p.pred_id, p.negate, first, (int32_t)p.arg1, 0u,
                                 (uint32_t)(p.pred_id == DSL_PRED_NET ? d.n_net++ : ds.n_sent++)};
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
  auto compile = [&](const dsl_predicate* src, int n, DevProg* dst, const char* name) {
    list_name = name;
    for (int i = 0; i < n; i++) {
      const int start = d.n_ops;
      int sp = 0;
      if (!emit(src[i], 0, &sp)) return false;
      dst[i] = DevProg{(int16_t)start, (int16_t)(d.n_ops - start)};
    }
    return true;
  };
  if (!compile(in.invariants, d.n_inv, d.inv, "invariants") || !compile(in.goals, d.n_goal, d.goal, "goals") ||
      !compile(in.prunes, d.n_prune, d.prune, "prunes")) {
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
    if (!compile(watches->watches, watches->n, d.watch, "watches")) {
      *why_out = why;
      return why.rfind("predicate not supported", 0) == 0 ? DSL_ERR_UNKNOWN_PREDICATE : DSL_ERR_ARG;
    }
    d.n_watch = watches->n;
    d.watch_net = d.n_net > net0 ? 1 : 0;
  }
  if (steps && steps->n != 0) {
    if (steps->n < 0 || steps->n > DSL_MAX_STEP_INVARIANTS)
      return *why_out = "step invariants: " + std::to_string(steps->n) + ", outside 0.." +
                        std::to_string(DSL_MAX_STEP_INVARIANTS), DSL_ERR_ARG;
    if (!step_out || !steps->preds || steps->n_pool < 0 || steps->n_pool > DSL_MAX_POOL || (steps->n_pool > 0 && !steps->pool))
      return *why_out = "step invariants: predicate counts out of range", DSL_ERR_ARG;
    pool = steps->pool;
    n_pool = steps->n_pool;
    const int ops0 = d.n_ops;
    in_step = true;
    const bool ok = compile(steps->preds, steps->n, ds.prog, "step invariants");
    in_step = false;
    if (!ok) {
      *why_out = why;
      return why.rfind("predicate not supported", 0) == 0 ? DSL_ERR_UNKNOWN_PREDICATE : DSL_ERR_ARG;
    }
    ds.n_step = steps->n;
    ds.op0 = ops0;
    ds.op1 = d.n_ops;
    d.n_ops = ops0;  // the step ops stay behind n_ops
  }
  *out = d;
  if (step_out) *step_out = ds;
  return DSL_OK;
}

}  // namespace dsl
