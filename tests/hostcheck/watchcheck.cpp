// tests/hostcheck/watchcheck.cpp -- TEST TOOL, not part of the product.
//
// The watches (dsl_set_watches: predicates that are only counted) on the host: a BFS with exact
// state equality (as protocheck.cpp) over the packed transition functions, under settings and
// watches given as the engine receives them and compiled through resolve_settings /
// check_field_leaves / check_net_leaves / set_pred_reads, the engine's own path. Every state the
// search discovers -- the start state, then every new successor whatever its verdict -- has its
// watches evaluated two ways:
//   * eval_watches on the delta view with the new records handed over (what k_level runs);
//   * an independent evaluation of the dsl_predicate trees on the MATERIALIZED state, written
//     here in plain C++: field leaves from the state's words, network leaves over the row's
//     records and the dropped records, the combinators with StatePredicate's three values. A
//     named leaf has no second implementation: it is P::eval on the whole materialized row, and
//     its truth is anchored by the oracle's goal searches (tests/test_watch.py).
// The two must agree on every (state, watch): "mismatch". The search itself must not depend on
// the watches: it is run a second time without them and must give the same per_depth and end
// ("search_changed"). One JSON line: per_depth, the census (per watch, one count per entry of
// per_depth), how many evaluations were true per watch, mismatch, errors.
// Built also with -fsanitize=undefined (the width-32 masks and the 64-bit shifts).
//
// usage: watchcheck <scenario name> <blob>    blob = dsl_protocol_desc, dsl_settings, int32 n_watches,
//          int32 n_pool, dsl_predicate[DSL_MAX_WATCHES], dsl_predicate[DSL_MAX_POOL], int32 n_dropped,
//          int32 start depth, int32 start state bytes (0: the initial state), int32 0,
//          uint64[n_dropped], the start state (tests/watch_cases.py writes it)
//        watchcheck refusals                  the host's refusals of bad watches (resolve_settings)
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <iterator>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../dslabs_amd/csrc/protocols/all.hpp"
#include "../../dslabs_amd/csrc/settings.hpp"

using namespace dsl;

namespace {

struct Input {
  dsl_protocol_desc desc;
  dsl_settings hs;
  int32_t n_watches = 0, n_pool = 0;
  dsl_predicate watches[DSL_MAX_WATCHES];
  dsl_predicate pool[DSL_MAX_POOL];
  int32_t depth0 = 0;
  std::vector<uint64_t> dropped;
  std::vector<uint8_t> start;
};

// ---- the independent evaluation (three-valued: 0 false, 1 true, 2 threw) --------------------------
uint32_t ref_field(const uint32_t* st, int node_words, uint32_t desc) {
  const int node = (int)((desc >> 22) & 31u), bit = (int)(desc & 0xffffu), width = (int)((desc >> 16) & 63u);
  const uint64_t word = st[node * node_words + bit / 32];
  return (uint32_t)((word >> (bit % 32)) & ((1ull << width) - 1ull));  // 64-bit: width 32 is no special case
}
bool ref_cmp(int cmp, uint64_t a, uint64_t b) {
  switch (cmp) {
    case DSL_CMP_EQ: return a == b;
    case DSL_CMP_NE: return a != b;
    case DSL_CMP_LT: return a < b;
    case DSL_CMP_LE: return a <= b;
    case DSL_CMP_GT: return a > b;
    default: return a >= b;
  }
}
bool ref_cond(const dsl_predicate& c, uint64_t rec) {
  const uint64_t a0 = (uint64_t)c.arg0;
  const int bit = (int)(a0 % 65536), width = (int)((a0 / 65536) % 64), cmp = (int)((a0 >> 32) % 8);
  uint64_t x = 0;  // bit by bit: no shift by the width, no mask
  for (int i = 0; i < width; i++)
    if (bit + i < 64 && ((rec >> (bit + i)) & 1ull)) x += 1ull << i;
  return ref_cmp(cmp, x, (uint64_t)c.arg1);
}
template <class P>
int ref_pred(const Input& in, const dsl_predicate& p, const uint32_t* st, const std::vector<uint64_t>& net,
             const typename P::Params& prm, const DevSettings& set) {
  int x;
  if (p.pred_id == DSL_PRED_FIELD) {
    const uint64_t a0 = (uint64_t)p.arg0;
    const uint32_t a = ref_field(st, P::kNodeWords, (uint32_t)a0);
    const uint32_t b = ((a0 >> 35) & 1u) ? ref_field(st, P::kNodeWords, (uint32_t)p.arg1) : (uint32_t)p.arg1;
    x = ref_cmp((int)((a0 >> 32) & 7u), a, b) ? 1 : 0;
  } else if (p.pred_id == DSL_PRED_NET) {
    x = 0;
    for (uint64_t rec : net) {
      bool all = true;
      for (int c = 0; c < (int)p.arg1; c++) all = all && ref_cond(in.pool[p.arg0 + c], rec);
      if (all) x = 1;
    }
  } else if (p.pred_id == DSL_PRED_AND || p.pred_id == DSL_PRED_OR || p.pred_id == DSL_PRED_IMPLIES) {
    // StatePredicate.and / or / implies (T/StatePredicate.java:397-431): a throwing left operand
    // throws; and(a, b) is a when a is false, else b; or(a, b) is a when a is true, else b;
    // implies(a, b) = or(negate(a), b); negate keeps a throw
    int a = ref_pred<P>(in, in.pool[p.arg0], st, net, prm, set);
    if (p.pred_id == DSL_PRED_IMPLIES && a != 2) a = !a;
    if (a == 2) x = 2;
    else if (p.pred_id == DSL_PRED_AND) x = a == 0 ? 0 : ref_pred<P>(in, in.pool[p.arg1], st, net, prm, set);
    else x = a == 1 ? 1 : ref_pred<P>(in, in.pool[p.arg1], st, net, prm, set);
  } else {
    // a named leaf: the protocol's own predicate on the whole materialized row (no delta view)
    NodeView whole{st, P::kNodeWords, -1, nullptr};
    if constexpr (NetPreds<P>::value) {
      whole.dropped = set.dropped();
      whole.ndropped = set.n_dropped;
    }
    const DevPred leaf{p.pred_id, 0, (int32_t)p.arg0, (int32_t)p.arg1, 0u, 0u};
    x = P::eval(leaf, whole, prm);
  }
  if (x != 2 && p.negate) x = !x;
  return x;
}

bool read_input(const char* path, Input* in) {
  std::ifstream f(path, std::ios::binary);
  std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t o = 0;
  auto take = [&](void* dst, size_t n) {
    if (o + n > b.size()) return false;
    if (n) std::memcpy(dst, b.data() + o, n);
    o += n;
    return true;
  };
  int32_t nd = 0, nstart = 0, pad = 0;
  if (!take(&in->desc, sizeof(in->desc)) || !take(&in->hs, sizeof(in->hs)) || !take(&in->n_watches, 4) ||
      !take(&in->n_pool, 4) || !take(in->watches, sizeof(in->watches)) || !take(in->pool, sizeof(in->pool)) ||
      !take(&nd, 4) || !take(&in->depth0, 4) || !take(&nstart, 4) || !take(&pad, 4) || nd < 0 || nstart < 0)
    return false;
  in->dropped.resize(nd);
  in->start.resize(nstart);
  return take(in->dropped.data(), 8 * (size_t)nd) && take(in->start.data(), (size_t)nstart) && o == b.size();
}

struct Outcome {
  std::vector<unsigned long long> per_depth;
  std::vector<std::vector<unsigned long long>> census;
  std::vector<unsigned long long> truths;
  long long mismatch = 0, evaluated = 0;
  int errors = 0, end = 0;  // end: 0 exhausted, else the terminal verdict
};

// watched: evaluate and count the watches (false: the same search without them)
template <class P>
Outcome bfs(const Input& in, bool watched) {
  Outcome o;
  const typename P::Params prm = P::from_desc(in.desc);
  DevSettings set;
  std::string why;
  const WatchList wl{in.watches, watched ? in.n_watches : 0, in.pool, watched ? in.n_pool : 0};
  if (!P::valid(prm) || resolve_settings(in.hs, P::num_nodes(prm), &P::known_predicate, &set, &why, &wl) ||
      !check_field_leaves<P>(set, &why) || !check_net_leaves<P>(set, &why)) {
    fprintf(stderr, "settings refused: %s\n", why.c_str());
    return o.errors++, o;
  }
  set_pred_reads<P>(set, prm);
  using S = typename P::State;
  using Rec = typename P::Rec;
  const int nw = set.n_watch;
  std::vector<Rec> dropped;
  for (uint64_t r : in.dropped) dropped.push_back((Rec)r);
  set.dropped_host = dropped.empty() ? nullptr : dropped.data();
  set.n_dropped = (int32_t)dropped.size();
  S init;
  if (!init_state<P>(init.w, prm)) return o.errors++, o;
  if (!in.start.empty()) {
    if (in.start.size() != sizeof(S)) return o.errors++, o;
    std::memcpy(init.w, in.start.data(), sizeof(S));
  }
  auto key = [](const S& s) { return std::string((const char*)s.w, sizeof(S)); };
  auto network = [&](const uint32_t* w) {
    std::vector<uint64_t> out;
    for (int j = 0; j < Net<P>::size(w); j++) out.push_back((uint64_t)Net<P>::at(w, j));
    for (uint64_t r : in.dropped) out.push_back(r);
    return out;
  };
  o.census.assign(nw, {});
  o.truths.assign(nw, 0);
  // counts one discovered state: `held` from eval_watches on its view, against the plain evaluation
  auto count = [&](uint32_t held, const uint32_t* st, size_t level) {
    const std::vector<uint64_t> net = network(st);
    for (int w = 0; w < nw; w++) {
      const bool a = (held >> w) & 1u, b = ref_pred<P>(in, in.watches[w], st, net, prm, set) == 1;
      o.evaluated++;
      if (a != b) o.mismatch++;
      if (o.census[w].size() <= level) o.census[w].resize(level + 1, 0);
      o.census[w][level] += a;
      o.truths[w] += a;
    }
  };
  struct Node {
    S s;
    int depth;
  };
  std::unordered_set<std::string> seen{key(init)};
  std::deque<Node> q;
  int tdepth = -1, pi = -1;
  o.per_depth.assign(1, 1);
  {
    const NodeView v0{init.w, P::kNodeWords, -1, nullptr};
    const int v = judge_view<P>(v0, prm, set, in.depth0, &pi);
    if (nw) count(eval_watches<P>(v0, prm, set), init.w, 0);
    if (v >= V_TERM_EXCEPTION) o.end = v;
    else q.push_back({init, in.depth0});  // the initial state is expanded also when pruned
  }
  while (!q.empty()) {
    const Node n = q.front();
    if (tdepth >= 0 && n.depth + 1 > tdepth) break;  // the terminal's level is finished, then the search ends
    q.pop_front();
    const int ne = count_events<P>(n.s.w, prm, set);
    for (int k = 0; k < ne; k++) {
      Delta<P> dl;
      const int rc = delta_step<P>(n.s.w, k, dl, prm, set);
      if (rc == STEP_NULL) continue;
      if (rc != STEP_OK) {  // none of these searches reaches an exception or an overflow
        o.errors++;
        continue;
      }
      const int dep = n.depth + 1;
      const size_t level = (size_t)(dep - in.depth0);
      S t;
      if (!materialize<P>(n.s.w, dl, t.w)) return o.errors++, o;
      if (!seen.insert(key(t)).second) continue;
      if (o.per_depth.size() <= level) o.per_depth.resize(level + 1, 0);
      o.per_depth[level]++;
      NodeView view{n.s.w, P::kNodeWords, dl.node, dl.nw};
      Rec news[P::kMaxSends];
      view.sends = news;
      view.nsends = delta_sends<P>(dl, news);
      // the verdict as the kernels reach it: incremental for successors of expanded non-initial parents
      const int v = judge_view<P>(view, prm, set, dep, &pi, n.depth > in.depth0);
      if (nw) {
        // the kernels' hit mask of the new records is computed from the delta's registers
        view.net_hits = delta_net_hits<P>(set, dl);
        view.sends = nullptr;
        view.nsends = 0;
        if constexpr (NetPreds<P>::value) {
          view.sends = news;
          view.nsends = delta_sends<P>(dl, news);
        }
        count(eval_watches<P>(view, prm, set), t.w, level);
      }
      if (v >= V_TERM_EXCEPTION) {
        if (tdepth < 0) tdepth = dep, o.end = v;
        continue;
      }
      if (v == V_PRUNED) continue;
      q.push_back({t, dep});
    }
  }
  for (auto& c : o.census) c.resize(o.per_depth.size(), 0);
  return o;
}

void print_vec(const std::vector<unsigned long long>& v) {
  printf("[");
  for (size_t i = 0; i < v.size(); i++) printf("%s%llu", i ? "," : "", v[i]);
  printf("]");
}

template <class P>
int run(const char* name, const Input& in) {
  const Outcome a = bfs<P>(in, true), b = bfs<P>(in, false);
  const bool changed = a.per_depth != b.per_depth || a.end != b.end;
  printf("{\"scenario\":\"%s\",\"end\":%d,\"per_depth\":", name, a.end);
  print_vec(a.per_depth);
  printf(",\"census\":[");
  for (size_t w = 0; w < a.census.size(); w++) {
    if (w) printf(",");
    print_vec(a.census[w]);
  }
  printf("],\"true\":");
  print_vec(a.truths);
  printf(",\"evaluated\":%lld,\"mismatch\":%lld,\"search_changed\":%d,\"errors\":%d}\n", a.evaluated, a.mismatch,
         changed ? 1 : 0, a.errors + b.errors);
  return a.errors || b.errors || a.mismatch || changed ? 1 : 0;
}

// ---- the host's refusals ------------------------------------------------------------------------
dsl_settings base_settings() {
  dsl_settings s{};
  s.max_depth = -1;
  s.max_time_ms = -1;
  s.network_active = 1;
  s.deliver_timers = 1;
  std::memset(s.link_active, -1, sizeof(s.link_active));
  std::memset(s.sender_active, -1, sizeof(s.sender_active));
  std::memset(s.receiver_active, -1, sizeof(s.receiver_active));
  std::memset(s.timers_active, -1, sizeof(s.timers_active));
  return s;
}
dsl_predicate field_leaf(int node, int bit, int width, int cmp, uint32_t k) {
  return dsl_predicate{DSL_PRED_FIELD, 0, DSL_FIELD_ARG0(DSL_FIELD_DESC(node, bit, width), cmp, 0), (int64_t)k};
}

int refusals() {
  using P = PingPongIR;  // 2 nodes of 6 words, 32-bit records
  dsl_protocol_desc d{};
  d.protocol = DSL_PROTO_PINGPONG_IR;
  const long long params[] = {1, 10, 1, 1};
  for (long long p : params) d.params[d.n_params++] = p;
  const typename P::Params prm = P::from_desc(d);
  const int nn = P::num_nodes(prm);
  const dsl_predicate named{DSL_PRED_CLIENTS_DONE, 0, 0, 0}, good = field_leaf(1, 96, 4, DSL_CMP_GE, 5);
  const dsl_predicate cond{DSL_PRED_REC_COND, 0, DSL_REC_ARG0(0, 4, DSL_CMP_GE), 1};
  int bad = 0;
  bool first = true;
  printf("{\"refusals\":[");
  // each case: settings, watches, pool; the call must fail with `want` in its text and leave a
  // DevSettings holding a sentinel untouched
  auto refuse = [&](const char* what, const dsl_settings& hs, const std::vector<dsl_predicate>& w,
                    const std::vector<dsl_predicate>& pool, const char* want, bool also_p = false) {
    DevSettings set;
    std::memset(&set, 0x5a, sizeof(set));
    DevSettings before;
    std::memcpy(&before, &set, sizeof(set));
    std::string why;
    const WatchList wl{w.data(), (int32_t)w.size(), pool.data(), (int32_t)pool.size()};
    int rc = resolve_settings(hs, nn, &P::known_predicate, &set, &why, &wl);
    bool untouched = std::memcmp(&before, &set, sizeof(set)) == 0;
    if (rc == DSL_OK && also_p) {  // the check that needs the protocol (the engine runs it before it keeps anything)
      rc = check_field_leaves<P>(set, &why) && check_net_leaves<P>(set, &why) ? DSL_OK : DSL_ERR_ARG;
      untouched = true;
    }
    const bool ok = rc == DSL_ERR_ARG && why.find(want) != std::string::npos && untouched;
    if (!ok) bad++;
    printf("%s{\"case\":\"%s\",\"rc\":%d,\"why\":\"%s\",\"untouched\":%s,\"ok\":%s}", first ? "" : ",", what, rc, why.c_str(),
           untouched ? "true" : "false", ok ? "true" : "false");
    first = false;
  };
  const dsl_settings plain = base_settings();
  refuse("nine watches", plain, std::vector<dsl_predicate>(9, named), {}, "outside 0..8");
  refuse("bad field descriptor", plain, {field_leaf(1, 30, 4, DSL_CMP_EQ, 1)}, {}, "straddles a 32-bit word");
  refuse("field beyond the node", plain, {field_leaf(1, 192, 1, DSL_CMP_EQ, 1)}, {}, "beyond the node", true);
  refuse("unknown node", plain, {field_leaf(2, 0, 4, DSL_CMP_EQ, 1)}, {}, "node index");
  refuse("record condition as a watch", plain, {cond}, {}, "used as a predicate or a combinator operand");
  refuse("combinator operand outside the pool", plain, {dsl_predicate{DSL_PRED_AND, 0, 0, 1}}, {good}, "combinator operand outside");
  {
    // settings plus watches past 64 ops: 16 + 16 + 16 single-leaf predicates, then 8 watches of 3 ops
    dsl_settings hs = base_settings();
    for (int i = 0; i < DSL_MAX_PREDICATES; i++) hs.invariants[hs.n_invariants++] = hs.goals[hs.n_goals++] = hs.prunes[hs.n_prunes++] = good;
    std::vector<dsl_predicate> w, pool{good, good};
    for (int i = 0; i < 8; i++) w.push_back(dsl_predicate{DSL_PRED_OR, 0, 0, 1});
    refuse("past 64 ops", hs, w, pool, "predicate programs too long");
  }
  {
    // settings plus watches past 32 network conditions: 3 leaves of 8 in the settings, 2 of 8 in the watches
    dsl_settings hs = base_settings();
    for (int i = 0; i < 8; i++) hs.pool[hs.n_pool++] = cond;
    for (int i = 0; i < 3; i++) hs.goals[hs.n_goals++] = dsl_predicate{DSL_PRED_NET, 0, 0, 8};
    const std::vector<dsl_predicate> pool(8, cond), w(2, dsl_predicate{DSL_PRED_NET, 0, 0, 8});
    refuse("past 32 network conditions", hs, w, pool, "more than 32 conditions in all");
    // ... and the same settings take one such watch (24 + 8 = 32)
    DevSettings set;
    std::string why;
    const WatchList wl{w.data(), 1, pool.data(), 8};
    const int rc = resolve_settings(hs, nn, &P::known_predicate, &set, &why, &wl);
    const bool ok = rc == DSL_OK && set.n_watch == 1 && set.watch_net == 1 && set.n_net == 4 && set.ops[set.watch[0].start].pad == 3u;
    if (!ok) bad++;
    printf(",{\"case\":\"32 conditions fit\",\"rc\":%d,\"ok\":%s}", rc, ok ? "true" : "false");
  }
  int flat = -1, n_ops = -1, watch_len = -1;
  {
    // flat is the settings' alone: single-leaf invariants with a watch that is a tree
    dsl_settings hs = base_settings();
    hs.invariants[hs.n_invariants++] = dsl_predicate{DSL_PRED_RESULTS_OK, 0, 0, 0};
    hs.prunes[hs.n_prunes++] = named;
    const std::vector<dsl_predicate> pool{good, named}, w{dsl_predicate{DSL_PRED_IMPLIES, 1, 0, 1}, good};
    DevSettings set;
    std::string why;
    const WatchList wl{w.data(), 2, pool.data(), 2};
    const int rc = resolve_settings(hs, nn, &P::known_predicate, &set, &why, &wl);
    DevSettings none;
    const int rc0 = resolve_settings(hs, nn, &P::known_predicate, &none, &why);
    flat = rc == DSL_OK ? set.flat : -1;
    n_ops = set.n_ops;
    watch_len = set.watch[0].len;
    if (rc || rc0 || set.flat != 1 || none.flat != 1 || none.n_watch != 0 || set.n_watch != 2 || set.watch[0].start != 2 ||
        set.watch[0].len != 5 || set.watch[1].start != 7 || set.watch[1].len != 1 || set.n_ops != 8 || set.watch_net != 0)
      bad++;
  }
  printf("],\"flat\":%d,\"n_ops\":%d,\"watch0_len\":%d,\"bad\":%d}\n", flat, n_ops, watch_len, bad);
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "refusals") return refusals();
  if (argc != 3) return fprintf(stderr, "usage: watchcheck <scenario> <blob> | watchcheck refusals\n"), 2;
  Input in;
  if (!read_input(argv[2], &in)) return fprintf(stderr, "watchcheck: bad blob\n"), 2;
  switch (in.desc.protocol) {
    case DSL_PROTO_PINGPONG: return run<PingPong>(argv[1], in);
    case DSL_PROTO_MULTIPAXOS: return run<MultiPaxos>(argv[1], in);
    case DSL_PROTO_PB: return run<PB>(argv[1], in);
    case DSL_PROTO_PINGPONG_IR: return run<PingPongIR>(argv[1], in);
    case DSL_PROTO_MULTIPAXOS_IR: return run<MultiPaxosIR>(argv[1], in);
    case DSL_PROTO_PB_IR: return run<PBIR>(argv[1], in);
    default: return fprintf(stderr, "watchcheck: protocol %d is not wired in\n", in.desc.protocol), 2;
  }
}
