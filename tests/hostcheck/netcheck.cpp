// tests/hostcheck/netcheck.cpp -- TEST TOOL, not part of the product.
//
// The generic network leaf (DSL_PRED_NET) on the host: small BFSs (exact state equality, as
// protocheck.cpp) of PBIR, the hand-written PB, MultiPaxosIR, PingPongIR and AmoKVIR under
// settings whose predicates are network leaves -- single, negated, inside and / or / implies,
// as invariant, goal and prune, one search over a dropped network -- given as dsl_settings through
// resolve_settings / check_net_leaves / set_pred_reads, the engine's own path. Every successor is
// judged three ways:
//   * judge_view on the delta view with the new records handed over (what the kernels run), full;
//   * the same with incremental = true (successors of expanded non-initial parents): must equal
//     the full verdict ("judge_mismatch");
//   * an independent evaluation of the dsl_settings predicate trees over the MATERIALIZED row's
//     records and the dropped records, written here in plain C++ (none of rec_matches): must
//     equal it too ("ref_mismatch").
// It counts the successors where a new record turned a leaf from false to true ("flips") and the
// (successor, leaf) pairs the incremental judge kept as unchanged ("skipped"): both must be above
// 0, or the run checks nothing. One JSON line per scenario (with the terminal depth and the
// number of distinct terminal states of the level that ended the search) and a total.
// Built also with -fsanitize=undefined: the width-32 mask and the 64-bit shift are the hazards.
//
// usage: netcheck
#include <cstdio>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../dslabs_amd/csrc/protocols/all.hpp"
#include "../../dslabs_amd/csrc/settings.hpp"

using namespace dsl;

namespace {

struct Counts {
  long long succ = 0, judged = 0, judge_mismatch = 0, ref_mismatch = 0, terminal = 0, pruned = 0, incremental = 0;
  long long flips = 0, skipped = 0, states = 0;
  int errors = 0, terminal_depth = -1;
};

// ---- the independent evaluation -------------------------------------------------------------------
bool ref_cond(const dsl_predicate& c, uint64_t rec) {
  const uint64_t a0 = (uint64_t)c.arg0;
  const int bit = (int)(a0 % 65536), width = (int)((a0 / 65536) % 64), cmp = (int)((a0 >> 32) % 8);
  uint64_t x = 0;  // bit by bit: no shift by the width, no mask
  for (int i = 0; i < width; i++)
    if (bit + i < 64 && ((rec >> (bit + i)) & 1ull)) x += 1ull << i;
  const uint64_t k = (uint64_t)c.arg1;
  switch (cmp) {
    case DSL_CMP_EQ: return x == k;
    case DSL_CMP_NE: return x != k;
    case DSL_CMP_LT: return x < k;
    case DSL_CMP_LE: return x <= k;
    case DSL_CMP_GT: return x > k;
    default: return x >= k;
  }
}
bool ref_pred(const dsl_settings& s, const dsl_predicate& p, const std::vector<uint64_t>& net) {
  bool x = false;
  if (p.pred_id == DSL_PRED_NET) {
    for (uint64_t rec : net) {
      bool all = true;
      for (int c = 0; c < (int)p.arg1; c++) all = all && ref_cond(s.pool[p.arg0 + c], rec);
      if (all) x = true;
    }
  } else {
    const bool a = ref_pred(s, s.pool[p.arg0], net);
    const bool b = ref_pred(s, s.pool[p.arg1], net);
    x = p.pred_id == DSL_PRED_AND ? (a && b) : p.pred_id == DSL_PRED_OR ? (a || b) : (!a || b);
  }
  return p.negate ? !x : x;
}
int ref_judge(const dsl_settings& s, const std::vector<uint64_t>& net, int depth, int* pi) {
  for (int i = 0; i < s.n_invariants; i++)
    if (!ref_pred(s, s.invariants[i], net)) return *pi = i, (int)V_TERM_INVARIANT;
  for (int i = 0; i < s.n_goals; i++)
    if (ref_pred(s, s.goals[i], net)) return *pi = i, (int)V_TERM_GOAL;
  for (int i = 0; i < s.n_prunes; i++)
    if (ref_pred(s, s.prunes[i], net)) return (int)V_PRUNED;
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
struct Cond {
  int bit, width, cmp;
  uint32_t k;
};
dsl_predicate net(dsl_settings& s, std::initializer_list<Cond> conds, bool negate = false) {
  const int first = s.n_pool;
  for (const Cond& c : conds)
    s.pool[s.n_pool++] = dsl_predicate{DSL_PRED_REC_COND, 0, DSL_REC_ARG0(c.bit, c.width, c.cmp), (int64_t)c.k};
  return dsl_predicate{DSL_PRED_NET, negate ? 1 : 0, first, (int64_t)conds.size()};
}
dsl_predicate comb(dsl_settings& s, int id, const dsl_predicate& a, const dsl_predicate& b, bool negate = false) {
  s.pool[s.n_pool] = a;
  s.pool[s.n_pool + 1] = b;
  s.n_pool += 2;
  return dsl_predicate{id, negate ? 1 : 0, s.n_pool - 2, s.n_pool - 1};
}

template <class P>
std::vector<uint64_t> network_of(const uint32_t* w, const std::vector<typename P::Rec>& dropped) {
  std::vector<uint64_t> out;
  for (int j = 0; j < Net<P>::size(w); j++) out.push_back((uint64_t)Net<P>::at(w, j));
  for (auto r : dropped) out.push_back((uint64_t)r);
  return out;
}

// prefix: event 0 is applied this many times to the initial state, then every pending record moves
// to the dropped set (SearchState.dropPendingMessages) and the search starts there.
template <class P>
Counts run(const char* name, const dsl_protocol_desc& d, const dsl_settings& hs, int prefix = 0) {
  Counts c;
  const typename P::Params prm = P::from_desc(d);
  DevSettings set;
  std::string why;
  if (!P::valid(prm) || resolve_settings(hs, P::num_nodes(prm), &P::known_predicate, &set, &why) ||
      !check_field_leaves<P>(set, &why) || !check_net_leaves<P>(set, &why)) {
    fprintf(stderr, "%s: settings refused: %s\n", name, why.c_str());
    c.errors++;
    return c;
  }
  set_pred_reads<P>(set, prm);
  using S = typename P::State;
  using Rec = typename P::Rec;
  struct Node {
    S s;
    int depth;
  };
  auto key = [](const S& s) { return std::string((const char*)s.w, sizeof(S)); };
  S init;
  if (!init_state<P>(init.w, prm)) return c.errors++, c;
  std::vector<Rec> dropped;
  if (prefix > 0) {
    for (int i = 0; i < prefix; i++) {
      S nx;
      if (full_step<P>(init.w, 0, nx.w, prm, set) != STEP_OK) return c.errors++, c;
      init = nx;
    }
    for (int j = 0; j < Net<P>::size(init.w); j++) dropped.push_back(Net<P>::at(init.w, j));
    for (int j = 0; j < (int)dropped.size(); j++) Net<P>::put(init.w, j, 0);
    init.w[Layout<P>::kNetCount] = 0;
    set.dropped_host = dropped.data();
    set.n_dropped = (int32_t)dropped.size();
  }
  std::unordered_set<std::string> seen{key(init)};
  std::deque<Node> q;
  int pi = -1, tdepth = -1;
  {
    const NodeView v0{init.w, P::kNodeWords, -1, nullptr};
    int rpi = -1;
    const int v = judge_view<P>(v0, prm, set, 0, &pi), r = ref_judge(hs, network_of<P>(init.w, dropped), 0, &rpi);
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
      Rec news[P::kMaxSends];
      view.sends = news;
      view.nsends = delta_sends<P>(dl, news);
      int pf = -1, pr = -1;
      const int v = judge_view<P>(view, prm, set, dep, &pf);
      const int r = ref_judge(hs, network_of<P>(t.w, dropped), dep, &pr);
      if (v != r || (v >= V_TERM_EXCEPTION && pf != pr)) c.ref_mismatch++;
      {  // the materialized state itself (no new records: a full scan) must judge the same
        const NodeView whole{t.w, P::kNodeWords, -1, nullptr};
        int pw = -1;
        const int vw = judge_view<P>(whole, prm, set, dep, &pw);
        if (vw != v || (v >= V_TERM_EXCEPTION && pw != pf)) c.ref_mismatch++;
      }
      {  // what the new records did to each leaf: the register mask must be the list's
        const uint32_t hits = sends_net_hits<P>(set, news, view.nsends);
        if (hits != delta_net_hits<P>(set, dl)) c.judge_mismatch++;
        const uint32_t before = row_net_hits<P>(set, n.s.w);  // the parent's own leaf values
        bool flipped = false;
        for (int i = 0; i < set.n_ops; i++) {
          const DevPred& op = set.ops[i];
          if (op.id != DSL_PRED_NET) continue;
          if ((hits >> op.pad) & 1u) flipped |= !((before >> op.pad) & 1u);
          else if (n.depth > 0) c.skipped++;
        }
        c.flips += flipped;
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
  c.states = (long long)seen.size();
  c.terminal_depth = tdepth;
  printf("{\"scenario\":\"%s\",\"successors\":%lld,\"judged\":%lld,\"states\":%lld,\"incremental\":%lld,"
         "\"judge_mismatch\":%lld,\"ref_mismatch\":%lld,\"terminal\":%lld,\"terminal_depth\":%d,\"pruned\":%lld,"
         "\"flips\":%lld,\"skipped\":%lld,\"errors\":%d}\n",
         name, c.succ, c.judged, c.states, c.incremental, c.judge_mismatch, c.ref_mismatch, c.terminal, c.terminal_depth,
         c.pruned, c.flips, c.skipped, c.errors);
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
  a.flips += b.flips;
  a.skipped += b.skipped;
  a.states += b.states;
  a.errors += b.errors;
}

dsl_protocol_desc desc_of(int id, std::initializer_list<long long> params) {
  dsl_protocol_desc d{};
  d.protocol = id;
  for (long long p : params) d.params[d.n_params++] = p;
  return d;
}

}  // namespace

int main() {
  Counts total;
  const int EQ = DSL_CMP_EQ, NE = DSL_CMP_NE, LT = DSL_CMP_LT, GE = DSL_CMP_GE, LE = DSL_CMP_LE, GT = DSL_CMP_GT;
  // lab2 primary-backup, 2 servers, 1 client, putget; 64-bit records, in the IR-generated and in the
  // hand-written protocol alike: type bits 60-63 (2 = ViewReply, 0 = Ping, 4 = Reply), from 57-59,
  // to 54-56 (viewserver 0, server1 1, server2 2, client1 3); ViewReply: num 0-3, p 4-5, b 6-7
  // (parameters as dslabs_amd.protocols.PBIR(2, 1, "putget").params() / PB(2, 1, "putget").params())
  const dsl_protocol_desc pbir = desc_of(DSL_PROTO_PB_IR, {2, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 5, -1, -1, -1, -1});
  const dsl_protocol_desc pb = desc_of(DSL_PROTO_PB, {2, 1, 2, 1, 0, 0, 3, 0, 0, 0, 5, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1});
  {
    // programs: initView's shape -- prune a later view and a wrong view 2, goal View(2, 1, 2) at the client
    dsl_settings s = base_settings(11);
    s.invariants[s.n_invariants++] =
        comb(s, DSL_PRED_IMPLIES, net(s, {{60, 4, EQ, 2}, {0, 4, GE, 2}}), net(s, {{60, 4, EQ, 2}, {0, 4, EQ, 1}}));
    s.prunes[s.n_prunes++] = net(s, {{60, 4, EQ, 2}, {0, 4, GE, 3}});
    s.prunes[s.n_prunes++] = comb(s, DSL_PRED_AND, net(s, {{60, 4, EQ, 2}, {0, 4, GE, 2}}),
                                  net(s, {{60, 4, EQ, 2}, {0, 4, EQ, 2}, {4, 2, EQ, 1}, {6, 2, EQ, 2}}, true));
    s.goals[s.n_goals++] = comb(s, DSL_PRED_AND, net(s, {{60, 4, EQ, 2}, {54, 3, EQ, 3}, {0, 4, EQ, 2}, {4, 2, EQ, 1}, {6, 2, EQ, 2}}),
                                net(s, {{60, 4, EQ, 2}, {0, 4, GE, 3}}, true));
    add(total, run<PBIR>("pbir_initview", pbir, s));
  }
  {
    // flat: hasViewReply(3) as a prune, a negated invariant, a goal on a Reply to the client
    dsl_settings s = base_settings(10);
    s.invariants[s.n_invariants++] = net(s, {{60, 4, EQ, 2}, {0, 4, GT, 3}}, true);
    s.goals[s.n_goals++] = net(s, {{60, 4, EQ, 4}, {54, 3, EQ, 3}, {0, 2, EQ, 2}});  // Reply(seq 2) to client1
    s.prunes[s.n_prunes++] = net(s, {{60, 4, EQ, 2}, {0, 4, GE, 3}});
    add(total, run<PB>("pb_flat", pb, s));
  }
  {
    // over a dropped network: after two deliveries everything pending is dropped (a ViewReply of
    // view 1 among it); "a ViewReply was sent" then holds through the dropped records alone
    dsl_settings s = base_settings(8);
    s.invariants[s.n_invariants++] = net(s, {{60, 4, EQ, 2}, {0, 4, GE, 1}});
    s.invariants[s.n_invariants++] = comb(s, DSL_PRED_OR, net(s, {{60, 4, EQ, 2}, {0, 4, LE, 1}}, true), net(s, {{60, 4, EQ, 0}}));
    s.prunes[s.n_prunes++] = net(s, {{60, 4, EQ, 0}, {57, 3, NE, 1}, {0, 4, GE, 1}});  // a Ping(>= 1) not from server1
    s.goals[s.n_goals++] = net(s, {{60, 4, EQ, 2}, {0, 4, GE, 2}});
    add(total, run<PB>("pb_dropped", pb, s, 2));
    add(total, run<PBIR>("pbir_dropped", pbir, s, 2));
  }
  // MultiPaxosIR, 3 servers, 2 clients, append-xy; 64-bit records, 12 sends per step: type bits 61-63
  // (3 = P1b, 4 = P2a, 6 = Decision), from 58-60, to 55-57 (servers 0-2, clients 3-4); P2a: round
  // 0-3, leader 4-5, slot 6-8, cmd 9-11; Decision: slot 0-2, cmd 3-5; P1b: l3 bits 28-38 (across bit 32)
  const dsl_protocol_desc mp = desc_of(DSL_PROTO_MULTIPAXOS_IR, {3, 2, 1, 1, 2, 0, 0, 2, 0, 0, 1, 0, 0, 2, 0, 0, -1, -1, -1, -1, -1, -1});
  {
    dsl_settings s = base_settings(-1);
    s.goals[s.n_goals++] = net(s, {{61, 3, EQ, 6}, {0, 3, EQ, 1}});  // a Decision for slot 1
    add(total, run<MultiPaxosIR>("mp_goal_decision", mp, s));
  }
  {
    dsl_settings s = base_settings(-1);
    s.invariants[s.n_invariants++] = net(s, {{61, 3, EQ, 4}, {58, 3, EQ, 1}}, true);  // never a P2a from server2
    add(total, run<MultiPaxosIR>("mp_inv_p2a", mp, s));
  }
  {
    // depth 6 under trees; a field across bit 32 of the record; a width-32 field of its upper half
    dsl_settings s = base_settings(6);
    s.invariants[s.n_invariants++] = comb(s, DSL_PRED_OR, net(s, {{61, 3, EQ, 3}, {28, 11, NE, 0}}, true), net(s, {{61, 3, EQ, 4}}));
    s.invariants[s.n_invariants++] = net(s, {{32, 32, GE, 0xfffffff0u}}, true);  // the upper half as one 32-bit field
    s.prunes[s.n_prunes++] = comb(s, DSL_PRED_AND, net(s, {{61, 3, EQ, 2}, {58, 3, EQ, 2}}), net(s, {{61, 3, EQ, 2}, {58, 3, EQ, 1}}));
    s.prunes[s.n_prunes++] = net(s, {{61, 3, EQ, 3}, {55, 3, EQ, 0}, {0, 4, GE, 1}});  // a P1b to server1
    add(total, run<MultiPaxosIR>("mp_trees_d6", mp, s));
  }
  // PingPongIR, 1 client x 10 pings; 32-bit records: type bit 31 (1 = PongReply), from 28-30, to
  // 25-27, value 0-3
  const dsl_protocol_desc pp = desc_of(DSL_PROTO_PINGPONG_IR, {1, 10, 1, 1});
  {
    dsl_settings s = base_settings(-1);
    s.goals[s.n_goals++] = net(s, {{31, 1, EQ, 1}, {0, 4, EQ, 3}});  // PongReply(3)
    add(total, run<PingPongIR>("pp_goal_pong3", pp, s));
  }
  {
    dsl_settings s = base_settings(-1);
    s.invariants[s.n_invariants++] = net(s, {{31, 1, EQ, 0}, {0, 4, GT, 10}}, true);
    s.invariants[s.n_invariants++] = net(s, {{0, 32, LT, 0x80000000u}});  // some PingRequest: the whole record as a field
    s.prunes[s.n_prunes++] = net(s, {{31, 1, EQ, 1}, {0, 4, GE, 5}});
    add(total, run<PingPongIR>("pp_prune_pong5", pp, s));
  }
  // AmoKVIR, 2 clients, diffkey3; 32-bit records: type bit 31 (1 = Reply), from 29-30, to 27-28
  // (server 0, clients 1-2), seq 0-1, result 2-25
  const dsl_protocol_desc kv = desc_of(DSL_PROTO_AMOKV_IR, {2, 3, 2, 2, 2, 2, 2, 2, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 2, 0,
                                                            1, 2, 0, 0, 0, 4, 264, 2316, 4, 264, 2316, -1, -1, -1});
  {
    dsl_settings s = base_settings(-1);
    s.invariants[s.n_invariants++] = comb(s, DSL_PRED_IMPLIES, net(s, {{31, 1, EQ, 1}, {0, 2, GE, 2}}), net(s, {{31, 1, EQ, 0}, {0, 2, GE, 2}}));
    s.goals[s.n_goals++] = net(s, {{31, 1, EQ, 1}, {27, 2, EQ, 2}, {0, 2, EQ, 3}});  // Reply(seq 3) to client2
    s.prunes[s.n_prunes++] = net(s, {{31, 1, EQ, 1}, {27, 2, EQ, 1}, {0, 2, EQ, 2}});  // Reply(seq 2) to client1
    add(total, run<AmoKVIR>("kv_goal_reply3", kv, s));
  }
  const bool ok = total.errors == 0 && total.judge_mismatch == 0 && total.ref_mismatch == 0 && total.terminal > 0 &&
                  total.pruned > 0 && total.incremental > 0 && total.flips > 0 && total.skipped > 0;
  printf("{\"total\":true,\"successors\":%lld,\"judged\":%lld,\"incremental\":%lld,\"judge_mismatch\":%lld,"
         "\"ref_mismatch\":%lld,\"terminal\":%lld,\"pruned\":%lld,\"flips\":%lld,\"skipped\":%lld,\"errors\":%d,\"ok\":%s}\n",
         total.succ, total.judged, total.incremental, total.judge_mismatch, total.ref_mismatch, total.terminal,
         total.pruned, total.flips, total.skipped, total.errors, ok ? "true" : "false");
  return ok ? 0 : 1;
}
