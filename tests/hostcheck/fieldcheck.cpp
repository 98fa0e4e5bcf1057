// tests/hostcheck/fieldcheck.cpp -- TEST TOOL, not part of the product.
//
// The generic field leaf (DSL_PRED_FIELD) on the host: for the IR-generated PingPong and
// Multi-Paxos it runs small BFSs (exact state equality, as protocheck.cpp) under settings whose
// predicates are field leaves -- a scalar, a list element, a sub-field, a field-field compare, a
// width-32 raw field, negated leaves and combinators -- given as dsl_settings through
// resolve_settings / check_field_leaves / set_pred_reads, the engine's own path. Every successor is
// judged three ways:
//   * judge_view on the delta view (what the kernels run), full;
//   * judge_view on the same view with incremental = true (successors of expanded non-initial
//     parents): must equal the full verdict ("judge_mismatch");
//   * an independent evaluation of the dsl_settings predicate trees on the MATERIALIZED state,
//     written here in plain C++ (no shared code with the judge): must equal it too ("ref_mismatch").
// It prints one JSON line with the mismatch counts (must be 0) and the successors a field leaf
// judged TERMINAL and PRUNED (must both be above 0). Built also with -fsanitize=undefined: the
// width-32 mask is the hazard.
//
// usage: fieldcheck
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../dslabs_amd/csrc/protocols/all.hpp"
#include "../../dslabs_amd/csrc/settings.hpp"

using namespace dsl;

namespace {

struct Counts {
  long long succ = 0, judged = 0, judge_mismatch = 0, ref_mismatch = 0, terminal = 0, pruned = 0, incremental = 0;
  int errors = 0;
};

// ---- the independent evaluation -------------------------------------------------------------------
uint32_t ref_field(const uint32_t* st, int node_words, uint32_t desc) {
  const int node = (int)((desc >> 22) & 31u), bit = (int)(desc & 0xffffu), width = (int)((desc >> 16) & 63u);
  const uint64_t word = st[node * node_words + bit / 32];
  return (uint32_t)((word >> (bit % 32)) & ((1ull << width) - 1ull));  // 64-bit: width 32 is no special case
}
bool ref_pred(const dsl_settings& s, const dsl_predicate& p, const uint32_t* st, int node_words) {
  bool x;
  if (p.pred_id == DSL_PRED_FIELD) {
    const uint64_t a0 = (uint64_t)p.arg0;
    const uint32_t a = ref_field(st, node_words, (uint32_t)a0);
    const uint32_t b = ((a0 >> 35) & 1u) ? ref_field(st, node_words, (uint32_t)p.arg1) : (uint32_t)p.arg1;
    switch ((int)((a0 >> 32) & 7u)) {
      case DSL_CMP_EQ: x = a == b; break;
      case DSL_CMP_NE: x = a != b; break;
      case DSL_CMP_LT: x = a < b; break;
      case DSL_CMP_LE: x = a <= b; break;
      case DSL_CMP_GT: x = a > b; break;
      default: x = a >= b; break;
    }
  } else {
    const bool a = ref_pred(s, s.pool[p.arg0], st, node_words);
    const bool b = ref_pred(s, s.pool[p.arg1], st, node_words);
    x = p.pred_id == DSL_PRED_AND ? (a && b) : p.pred_id == DSL_PRED_OR ? (a || b) : (!a || b);
  }
  return p.negate ? !x : x;
}
int ref_judge(const dsl_settings& s, const uint32_t* st, int node_words, int depth, int* pi) {
  for (int i = 0; i < s.n_invariants; i++)
    if (!ref_pred(s, s.invariants[i], st, node_words)) return *pi = i, (int)V_TERM_INVARIANT;
  for (int i = 0; i < s.n_goals; i++)
    if (ref_pred(s, s.goals[i], st, node_words)) return *pi = i, (int)V_TERM_GOAL;
  for (int i = 0; i < s.n_prunes; i++)
    if (ref_pred(s, s.prunes[i], st, node_words)) return (int)V_PRUNED;
  if (s.max_depth >= 0 && depth >= s.max_depth) return (int)V_PRUNED;
  return (int)V_VALID;
}

// ---- settings builders ----------------------------------------------------------------------------
dsl_settings base_settings(int max_depth) {
  dsl_settings s{};
  s.max_depth = max_depth;
  s.max_time_ms = -1;
  s.network_active = 1;
  s.deliver_timers = 1;
  std::memset(s.link_active, -1, sizeof(s.link_active));
  std::memset(s.sender_active, -1, sizeof(s.sender_active));
  std::memset(s.receiver_active, -1, sizeof(s.receiver_active));
  std::memset(s.timers_active, -1, sizeof(s.timers_active));
  return s;
}
dsl_predicate leaf(int node, int bit, int width, int cmp, uint32_t k, bool negate = false) {
  return dsl_predicate{DSL_PRED_FIELD, negate ? 1 : 0, DSL_FIELD_ARG0(DSL_FIELD_DESC(node, bit, width), cmp, 0),
                       (int64_t)k};
}
dsl_predicate leaf2(int node, int bit, int width, int cmp, int node2, int bit2, int width2, bool negate = false) {
  return dsl_predicate{DSL_PRED_FIELD, negate ? 1 : 0, DSL_FIELD_ARG0(DSL_FIELD_DESC(node, bit, width), cmp, 1),
                       (int64_t)DSL_FIELD_DESC(node2, bit2, width2)};
}
dsl_predicate comb(dsl_settings& s, int id, const dsl_predicate& a, const dsl_predicate& b) {
  s.pool[s.n_pool] = a;
  s.pool[s.n_pool + 1] = b;
  s.n_pool += 2;
  return dsl_predicate{id, 0, s.n_pool - 2, s.n_pool - 1};
}

template <class P>
Counts run(const char* name, const dsl_protocol_desc& d, const dsl_settings& hs) {
  Counts c;
  const typename P::Params prm = P::from_desc(d);
  DevSettings set;
  std::string why;
  if (!P::valid(prm) || resolve_settings(hs, P::num_nodes(prm), &P::known_predicate, &set, &why) ||
      !check_field_leaves<P>(set, &why)) {
    fprintf(stderr, "%s: settings refused: %s\n", name, why.c_str());
    c.errors++;
    return c;
  }
  set_pred_reads<P>(set, prm);
  using S = typename P::State;
  struct Node {
    S s;
    int depth;
  };
  auto key = [](const S& s) { return std::string((const char*)s.w, sizeof(S)); };
  S init;
  if (!init_state<P>(init.w, prm)) return c.errors++, c;
  std::unordered_set<std::string> seen{key(init)};
  std::deque<Node> q;
  int pi = -1, tdepth = -1;
  {
    const NodeView v0{init.w, P::kNodeWords, -1, nullptr};
    int rpi = -1;
    const int v = judge_view<P>(v0, prm, set, 0, &pi), r = ref_judge(hs, init.w, P::kNodeWords, 0, &rpi);
    if (v != r || (v >= V_TERM_EXCEPTION && pi != rpi)) c.ref_mismatch++;
    if (v < V_TERM_EXCEPTION) q.push_back({init, 0});  // the initial state is expanded also when pruned
  }
  while (!q.empty()) {
    const Node n = q.front();
    if (tdepth >= 0 && n.depth + 1 > tdepth) break;
    q.pop_front();
    const int ne = count_events<P>(n.s.w, prm, set);
    for (int k = 0; k < ne; k++) {
      Delta<P> dl;
      const int rc = delta_step<P>(n.s.w, k, dl, prm, set);
      if (rc == STEP_NULL) continue;
      if (rc != STEP_OK) {  // none of these searches reaches an exception or an overflow
        c.errors++;
        continue;
      }
      c.succ++;
      const int dep = n.depth + 1;
      S t;
      if (!materialize<P>(n.s.w, dl, t.w)) return c.errors++, c;
      if (!seen.insert(key(t)).second) continue;
      c.judged++;
      NodeView view{n.s.w, P::kNodeWords, dl.node, dl.nw};
      int pf = -1, pr = -1;
      const int v = judge_view<P>(view, prm, set, dep, &pf);
      const int r = ref_judge(hs, t.w, P::kNodeWords, dep, &pr);
      if (v != r || (v >= V_TERM_EXCEPTION && pf != pr)) c.ref_mismatch++;
      {  // the materialized state itself (no changed node) must judge the same
        const NodeView whole{t.w, P::kNodeWords, -1, nullptr};
        int pw = -1;
        const int vw = judge_view<P>(whole, prm, set, dep, &pw);
        if (vw != v || (v >= V_TERM_EXCEPTION && pw != pf)) c.ref_mismatch++;
      }
      if (n.depth > 0) {  // the kernels' incremental judge: successors of expanded non-initial parents
        int p2 = -1;
        const int v2 = judge_view<P>(view, prm, set, dep, &p2, true);
        c.incremental++;
        if (v2 != v || (v >= V_TERM_EXCEPTION && p2 != pf)) c.judge_mismatch++;
      }
      if (v >= V_TERM_EXCEPTION) {
        c.terminal++;
        if (tdepth < 0) tdepth = dep;
        continue;
      }
      if (v == V_PRUNED) {
        if (!(hs.max_depth >= 0 && dep >= hs.max_depth)) c.pruned++;  // by a prune predicate, not by maxDepth
        continue;
      }
      q.push_back({t, dep});
    }
  }
  printf("{\"scenario\":\"%s\",\"successors\":%lld,\"judged\":%lld,\"incremental\":%lld,\"judge_mismatch\":%lld,"
         "\"ref_mismatch\":%lld,\"terminal\":%lld,\"pruned\":%lld,\"errors\":%d}\n",
         name, c.succ, c.judged, c.incremental, c.judge_mismatch, c.ref_mismatch, c.terminal, c.pruned, c.errors);
  return c;
}

void add(Counts& a, const Counts& b) {
  a.succ += b.succ;
  a.judged += b.judged;
  a.judge_mismatch += b.judge_mismatch;
  a.ref_mismatch += b.ref_mismatch;
  a.terminal += b.terminal;
  a.pruned += b.pruned;
  a.incremental += b.incremental;
  a.errors += b.errors;
}

}  // namespace

int main() {
  Counts total;
  // PingPongIR, 1 client x 10 pings (dslabs_amd/ir/specs/pingpong.py): client1 = node 1; ping bits
  // 0-3, pong 4-7, length(_timers) 8-11, length(_results) 96-99 (alone in word 3), _results[j] at
  // 128 + 4 j
  dsl_protocol_desc pp{};
  pp.protocol = DSL_PROTO_PINGPONG_IR;
  pp.n_params = 4;
  pp.params[0] = 1, pp.params[1] = 10, pp.params[2] = 1, pp.params[3] = 1;
  {
    // exhaustive with the prune "word 3 of client1 >= 4" (a width-32 raw field): flat leaves and programs mixed
    dsl_settings s = base_settings(-1);
    s.invariants[s.n_invariants++] = comb(s, DSL_PRED_OR, leaf(1, 96, 4, DSL_CMP_LE, 2), leaf(1, 128 + 8, 4, DSL_CMP_EQ, 3));
    s.invariants[s.n_invariants++] = leaf2(1, 0, 4, DSL_CMP_GE, 1, 4, 4);             // ping >= pong (one node)
    s.invariants[s.n_invariants++] = leaf(1, 96, 32, DSL_CMP_NE, 0xffffffffu);          // width 32
    s.invariants[s.n_invariants++] = leaf(1, 64, 32, DSL_CMP_GT, 0xfffffffeu, true);    // !(word 2 > 2^32 - 2)
    s.prunes[s.n_prunes++] = leaf(1, 96, 32, DSL_CMP_GE, 4);
    add(total, run<PingPongIR>("pp_prune_w32", pp, s));
  }
  {
    // flat: the goal length(_results) == 3 behind two invariants the search never violates
    dsl_settings s = base_settings(-1);
    s.invariants[s.n_invariants++] = leaf2(1, 4, 4, DSL_CMP_GT, 1, 0, 4, true);  // !(pong > ping)
    s.invariants[s.n_invariants++] = leaf(1, 8, 4, DSL_CMP_LT, 15);              // length(_timers) < 15
    s.goals[s.n_goals++] = leaf(1, 96, 4, DSL_CMP_EQ, 3);
    add(total, run<PingPongIR>("pp_goal_flat", pp, s));
  }
  {
    // RESULTS_OK restated: for every j, length <= j or results[j] == j + 1; goal: all ten received
    dsl_settings s = base_settings(-1);
    for (int j = 0; j < 10; j++)
      s.invariants[s.n_invariants++] =
          comb(s, DSL_PRED_OR, leaf(1, 96, 4, DSL_CMP_LE, (uint32_t)j), leaf(1, 128 + 4 * j, 4, DSL_CMP_EQ, (uint32_t)j + 1));
    s.goals[s.n_goals++] = leaf(1, 96, 4, DSL_CMP_EQ, 10);
    add(total, run<PingPongIR>("pp_results_ok", pp, s));
  }
  // MultiPaxosIR, 3 servers, 2 clients, append-xy (dslabs_amd/ir/specs/multipaxos.py; parameters as
  // dslabs_amd.protocols.MultiPaxosIR(3, 2, "append-xy").params()): servers = nodes 0-2; round bits
  // 0-3, leader 4-5, slotout 14-16; log[j] (11 bits: status 0-1, ballot 2-7, command 8-10) at
  // 32 + 32 (j / 2) + 11 (j % 2); clients = nodes 3-4, _results window = word 1
  dsl_protocol_desc mp{};
  mp.protocol = DSL_PROTO_MULTIPAXOS_IR;
  const long long mpp[] = {3, 2, 1, 1, 2, 0, 0, 2, 0, 0, 1, 0, 0, 2, 0, 0, -1, -1, -1, -1, -1, -1};
  mp.n_params = (int)(sizeof(mpp) / sizeof(mpp[0]));
  for (int i = 0; i < mp.n_params; i++) mp.params[i] = mpp[i];
  {
    // PaxosTest's implies(hasStatus(server1, 1, CHOSEN), hasCommand(server1, 1, X)) and the goal
    // hasStatus(server2, 1, CHOSEN), over sub-fields of log[0]
    dsl_settings s = base_settings(6);
    s.invariants[s.n_invariants++] =
        comb(s, DSL_PRED_IMPLIES, leaf(0, 32, 2, DSL_CMP_EQ, 2),
             comb(s, DSL_PRED_AND, leaf(0, 32, 2, DSL_CMP_NE, 0), leaf(0, 40, 3, DSL_CMP_EQ, 1)));
    s.goals[s.n_goals++] = leaf(1, 32, 2, DSL_CMP_EQ, 2);
    add(total, run<MultiPaxosIR>("mp_implies", mp, s));
  }
  {
    // depth 5 under prunes: a field-field compare across nodes, a width-32 raw field, a negated leaf
    dsl_settings s = base_settings(5);
    s.invariants[s.n_invariants++] = leaf2(0, 14, 3, DSL_CMP_LE, 0, 17, 3);       // server1: slotout <= slotin
    s.invariants[s.n_invariants++] = leaf(1, 32, 11, DSL_CMP_EQ, 2047, true);     // server2.log[0] != 2047
    s.prunes[s.n_prunes++] = leaf2(0, 0, 4, DSL_CMP_GT, 2, 0, 4);                 // server1.round > server3.round
    s.prunes[s.n_prunes++] = leaf(3, 32, 32, DSL_CMP_NE, 0);                      // client1 has a result (word 1)
    s.prunes[s.n_prunes++] = comb(s, DSL_PRED_AND, leaf2(1, 4, 2, DSL_CMP_EQ, 2, 4, 2), leaf(1, 0, 4, DSL_CMP_GE, 2));
    add(total, run<MultiPaxosIR>("mp_prunes", mp, s));
  }
  const bool ok = total.errors == 0 && total.judge_mismatch == 0 && total.ref_mismatch == 0 && total.terminal > 0 &&
                  total.pruned > 0 && total.incremental > 0;
  printf("{\"total\":true,\"successors\":%lld,\"judged\":%lld,\"incremental\":%lld,\"judge_mismatch\":%lld,"
         "\"ref_mismatch\":%lld,\"terminal\":%lld,\"pruned\":%lld,\"errors\":%d,\"ok\":%s}\n",
         total.succ, total.judged, total.incremental, total.judge_mismatch, total.ref_mismatch, total.terminal,
         total.pruned, total.errors, ok ? "true" : "false");
  return ok ? 0 : 1;
}
