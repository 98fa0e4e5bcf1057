// tests/hostcheck/emitcheck.cpp -- TEST TOOL, not part of the product.
//
// The mask rule of the row emitter (nodestate.hpp: delta_new_slots, emit_row_masked -- what
// kernels.hpp's wave_emit executes for a protocol of at most 64 records) against the rank rule
// (emit_row, which protocheck holds against materialize()):
//
//   emitcheck walk <proto> <params...> -- <inv ids> / <goal ids> / <prune ids> maxdepth
//     a host BFS with exact state equality, protocheck's arguments; on every successor the two rows
//     are compared (header and live records), and the mask with creator_record's
//   emitcheck crafted <proto>
//     the crafted rows of emit_cases.hpp
//
// One JSON object per run; tests/test_emit_rule.py judges it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <unordered_set>
#include <vector>

#include "emit_cases.hpp"

using namespace dsl;

// What differs between the two rules' rows: 1 header, 2 live records, 4 the mask against
// creator_record's, 8 the collision flag, 16 one rule refused the row and the other did not.
template <class P>
static int compare(const uint32_t* pw, const Delta<P>& d, bool equal_sends) {
  using L = Layout<P>;
  uint32_t a[L::kWords], b[L::kWords];
  uint64_t mask = 0;
  bool coll = false;
  const bool oka = emit_row<P>(pw, d, a), okb = emit_row_masked<P>(pw, d, b, &mask, &coll);
  if (oka != okb) return 16;
  if (!oka) return 0;
  int bad = 0;
  if (coll != equal_sends) bad |= 8;
  if (equal_sends) return bad;  // no row is defined: the caller raises an error
  for (int o = 0; o < L::kRecBase; o++)
    if (a[o] != b[o]) bad |= 1;
  const int cnt = Net<P>::size(a);
  for (int q = 0; q < cnt; q++)
    if (Net<P>::at(a, q) != Net<P>::at(b, q)) bad |= 2;
  uint32_t cw;
  uint64_t cm;
  creator_record<P>(pw, -1, d, &cw, &cm);
  if (cm != mask) bad |= 4;
  return bad;
}

template <class P>
static int crafted() {
  printf("{\"cases\":[");
  bool first = true;
  for (const auto& c : emitcases::crafted<P>()) {
    printf("%s{\"name\":\"%s\",\"n\":%d,\"m\":%d,\"equal_sends\":%s,\"bad\":%d}", first ? "" : ",", c.name.c_str(),
           Net<P>::size(c.pw), delta_new_count<P>(c.d), c.equal_sends ? "true" : "false",
           compare<P>(c.pw, c.d, c.equal_sends));
    first = false;
  }
  printf("]}\n");
  return 0;
}

template <class P>
static int walk(const dsl_protocol_desc& desc, DevSettings set) {
  typename P::Params prm = P::from_desc(desc);
  set_pred_reads<P>(set, prm);
  using S = typename P::State;
  struct Node {
    S s;
    int depth;
  };
  S init;
  if (!P::valid(prm) || !init_state<P>(init.w, prm)) {
    printf("{\"error\":\"bad fixture\"}\n");
    return 1;
  }
  auto key = [](const S& s) { return std::string((const char*)s.w, sizeof(S)); };
  std::unordered_set<std::string> seen{key(init)};
  std::deque<Node> q;
  std::vector<unsigned long long> per{1};
  long long succ = 0, multi = 0, mismatch = 0;
  int bad_bits = 0, pi = -1, tdepth = -1;
  NodeView v0{init.w, P::kNodeWords, -1, nullptr};
  if (judge_view<P>(v0, prm, set, 0, &pi) < V_TERM_EXCEPTION) q.push_back({init, 0});
  while (!q.empty()) {
    Node n = q.front();
    if (tdepth >= 0 && n.depth + 1 > tdepth) break;
    q.pop_front();
    const int ne = count_events<P>(n.s.w, prm, set);
    for (int k = 0; k < ne; k++) {
      Delta<P> dl;
      const int rc = delta_step<P>(n.s.w, k, dl, prm, set);
      if (rc == STEP_NULL) continue;
      const int d = n.depth + 1;
      if (rc == STEP_OVERFLOW) {
        printf("{\"error\":\"overflow\"}\n");
        return 1;
      }
      if (rc == STEP_EXCEPTION) {
        if ((int)per.size() <= d) per.resize(d + 1, 0);
        per[d]++;
        if (tdepth < 0) tdepth = d;
        continue;
      }
      succ++;
      if (delta_new_count<P>(dl) >= 2) multi++;
      const int bad = compare<P>(n.s.w, dl, false);
      if (bad) mismatch++, bad_bits |= bad;
      S t;
      if (!materialize<P>(n.s.w, dl, t.w)) {
        printf("{\"error\":\"overflow\"}\n");
        return 1;
      }
      if (!seen.insert(key(t)).second) continue;
      if ((int)per.size() <= d) per.resize(d + 1, 0);
      per[d]++;
      NodeView view{n.s.w, P::kNodeWords, dl.node, dl.nw};
      typename P::Rec news[P::kMaxSends];
      view.sends = news;
      view.nsends = delta_sends<P>(dl, news);
      const int v = judge_view<P>(view, prm, set, d, &pi);
      if (v >= V_TERM_EXCEPTION) {
        if (tdepth < 0) tdepth = d;
        continue;
      }
      if (v == V_PRUNED) continue;
      q.push_back({t, d});
    }
  }
  printf("{\"successors\":%lld,\"multi_send_rows\":%lld,\"mismatch\":%lld,\"bad_bits\":%d,\"per_depth\":[", succ, multi,
         mismatch, bad_bits);
  for (size_t i = 0; i < per.size(); i++) printf("%s%llu", i ? "," : "", per[i]);
  printf("]}\n");
  return 0;
}

// protocheck's settings arguments: predicate tokens [-]id[:arg0[:arg1]] or postfix programs
// joined by commas, the three lists separated by "/", then maxdepth
static DevSettings parse_settings(int argc, char** argv, int i) {
  DevSettings set{};
  for (int a = 0; a < DSL_MAX_NODES; a++) set.deliver[a] = 0xffffffffu;
  set.timer_mask = 0xffffffffu;
  set.all_deliver = 1;
  DevProg* lists[3] = {set.inv, set.goal, set.prune};
  int* counts[3] = {&set.n_inv, &set.n_goal, &set.n_prune};
  int which = 0;
  for (; i < argc - 1; i++) {
    if (strcmp(argv[i], "/") == 0) {
      which++;
      continue;
    }
    const int start = set.n_ops;
    for (const char* tok = argv[i]; *tok;) {
      const char* end = strchr(tok, ',');
      std::string t(tok, end ? (size_t)(end - tok) : strlen(tok));
      DevPred p{};
      if (t == "and") p.id = kOpAnd;
      else if (t == "or") p.id = kOpOr;
      else if (t == "not") p.id = kOpNot;
      else {
        int id = 0, a0 = 0, a1 = 0;
        sscanf(t.c_str(), "%d:%d:%d", &id, &a0, &a1);
        p.negate = id < 0;
        p.id = id < 0 ? -id : id;
        p.arg0 = a0;
        p.arg1 = a1;
      }
      set.ops[set.n_ops++] = p;
      tok = end ? end + 1 : tok + t.size();
    }
    lists[which][(*counts[which])++] = DevProg{(int16_t)start, (int16_t)(set.n_ops - start)};
  }
  set.max_depth = atoi(argv[argc - 1]);
  return set;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const bool is_walk = strcmp(argv[1], "walk") == 0;
  if (!is_walk && strcmp(argv[1], "crafted") != 0) return 2;
  dsl_protocol_desc d{};
  int i = 2;
  d.protocol = atoi(argv[i++]);
  DevSettings set{};
  if (is_walk) {
    while (i < argc && strcmp(argv[i], "--") != 0) d.params[d.n_params++] = atoll(argv[i++]);
    set = parse_settings(argc, argv, i + 1);
  }
  switch (d.protocol) {  // the protocols whose rows wave_emit writes by the mask rule (kNetCap <= 64)
    case DSL_PROTO_SIPAXOS: return is_walk ? walk<SIPaxos>(d, set) : crafted<SIPaxos>();
    case DSL_PROTO_MULTIPAXOS: return is_walk ? walk<MultiPaxos>(d, set) : crafted<MultiPaxos>();
    case DSL_PROTO_AMOKV: return is_walk ? walk<AmoKV>(d, set) : crafted<AmoKV>();
    case DSL_PROTO_PB: return is_walk ? walk<PB>(d, set) : crafted<PB>();
    case DSL_PROTO_MINITEST: return is_walk ? walk<MiniTest>(d, set) : crafted<MiniTest>();
    case DSL_PROTO_AMOKV_IR: return is_walk ? walk<AmoKVIR>(d, set) : crafted<AmoKVIR>();
    case DSL_PROTO_MULTIPAXOS_IR: return is_walk ? walk<MultiPaxosIR>(d, set) : crafted<MultiPaxosIR>();
    case DSL_PROTO_PB_IR: return is_walk ? walk<PBIR>(d, set) : crafted<PBIR>();
  }
  return 2;
}
