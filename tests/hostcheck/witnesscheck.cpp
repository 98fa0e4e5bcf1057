// tests/hostcheck/witnesscheck.cpp -- TEST TOOL, not part of the product.
//
// The witnesses of the watches (dsl_set_watch_witnesses) on the host: the BFS of watchcheck.cpp --
// exact state equality over the packed transition functions, the settings and watches compiled
// through the engine's own path -- which per watch records
//   * the first depth at which a newly discovered state held it,
//   * how many states of that depth held it,
//   * the holder with the smallest 128-bit fingerprint in (hi, lo) order (full_fingerprint of the
//     materialized state): hi, lo, the packed state as hex, and the length of its trace (BFS: the
//     number of events from the start state, a shortest trace).
// The holder is computed twice, as watchcheck computes the census twice: from eval_watches on the
// delta view (what the kernels run) and from the plain C++ evaluation of the predicate trees on
// the materialized state (ref_pred). The two must agree ("disagree": 0). One JSON line.
// Built also with -fsanitize=undefined.
//
// usage: witnesscheck <scenario name> <blob>    the blob watchcheck reads (tests/watch_cases.py blob)
//
// The input format, the reader and the plain evaluation are watchcheck.cpp's, taken whole (its
// main renamed): one copy of the reference evaluation for both tools.
#define main watchcheck_main
#include "watchcheck.cpp"
#undef main

namespace {

struct Holder {
  long long first = -1;  // level (depth - start depth) of the first hit
  unsigned long long count = 0;
  Fp fp{0, 0};
  std::vector<uint32_t> state;
  void take(long long level, const Fp& f, const uint32_t* st, size_t words) {
    if (first >= 0 && level != first) return;  // BFS order: a later level
    if (first < 0) first = level;
    if (count++ == 0 || f.hi < fp.hi || (f.hi == fp.hi && f.lo < fp.lo)) {
      fp = f;
      state.assign(st, st + words);
    }
  }
};

template <class P>
int witnesses(const char* name, const Input& in) {
  const typename P::Params prm = P::from_desc(in.desc);
  DevSettings set;
  std::string why;
  const WatchList wl{in.watches, in.n_watches, in.pool, in.n_pool};
  if (!P::valid(prm) || resolve_settings(in.hs, P::num_nodes(prm), &P::known_predicate, &set, &why, &wl) ||
      !check_field_leaves<P>(set, &why) || !check_net_leaves<P>(set, &why))
    return fprintf(stderr, "settings refused: %s\n", why.c_str()), 1;
  set_pred_reads<P>(set, prm);
  using S = typename P::State;
  using Rec = typename P::Rec;
  const int nw = set.n_watch;
  std::vector<Rec> dropped;
  for (uint64_t r : in.dropped) dropped.push_back((Rec)r);
  set.dropped_host = dropped.empty() ? nullptr : dropped.data();
  set.n_dropped = (int32_t)dropped.size();
  S init;
  int errors = 0;
  if (!init_state<P>(init.w, prm)) return 1;
  if (!in.start.empty()) {
    if (in.start.size() != sizeof(S)) return 1;
    std::memcpy(init.w, in.start.data(), sizeof(S));
  }
  auto key = [](const S& s) { return std::string((const char*)s.w, sizeof(S)); };
  auto network = [&](const uint32_t* w) {
    std::vector<uint64_t> out;
    for (int j = 0; j < Net<P>::size(w); j++) out.push_back((uint64_t)Net<P>::at(w, j));
    for (uint64_t r : in.dropped) out.push_back(r);
    return out;
  };
  std::vector<Holder> dv(nw), pl(nw);  // by the delta view, by the plain evaluation
  auto visit = [&](uint32_t held, const uint32_t* st, long long level) {
    const std::vector<uint64_t> net = network(st);
    const Fp f = full_fingerprint<P>(st);
    for (int w = 0; w < nw; w++) {
      if ((held >> w) & 1u) dv[w].take(level, f, st, sizeof(S) / 4);
      if (ref_pred<P>(in, in.watches[w], st, net, prm, set) == 1) pl[w].take(level, f, st, sizeof(S) / 4);
    }
  };
  struct Node {
    S s;
    int depth;
  };
  std::unordered_set<std::string> seen{key(init)};
  std::deque<Node> q;
  int tdepth = -1, pi = -1;
  std::vector<unsigned long long> per_depth(1, 1);
  {
    const NodeView v0{init.w, P::kNodeWords, -1, nullptr};
    const int v = judge_view<P>(v0, prm, set, in.depth0, &pi);
    visit(eval_watches<P>(v0, prm, set), init.w, 0);
    if (v < V_TERM_EXCEPTION) q.push_back({init, in.depth0});
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
        errors++;
        continue;
      }
      const int dep = n.depth + 1;
      const size_t level = (size_t)(dep - in.depth0);
      S t;
      if (!materialize<P>(n.s.w, dl, t.w)) return 1;
      if (!seen.insert(key(t)).second) continue;
      if (per_depth.size() <= level) per_depth.resize(level + 1, 0);
      per_depth[level]++;
      NodeView view{n.s.w, P::kNodeWords, dl.node, dl.nw};
      Rec news[P::kMaxSends];
      view.sends = news;
      view.nsends = delta_sends<P>(dl, news);
      const int v = judge_view<P>(view, prm, set, dep, &pi, n.depth > in.depth0);
      view.net_hits = delta_net_hits<P>(set, dl);  // as the kernels hand it over (watchcheck.cpp)
      if constexpr (!NetPreds<P>::value) {
        view.sends = nullptr;
        view.nsends = 0;
      }
      visit(eval_watches<P>(view, prm, set), t.w, (long long)level);
      if (v >= V_TERM_EXCEPTION) {
        if (tdepth < 0) tdepth = dep;
        continue;
      }
      if (v == V_PRUNED) continue;
      q.push_back({t, dep});
    }
  }
  int disagree = 0;
  printf("{\"scenario\":\"%s\",\"per_depth\":", name);
  print_vec(per_depth);
  printf(",\"witnesses\":[");
  for (int w = 0; w < nw; w++) {
    const Holder &a = dv[w], &b = pl[w];
    if (a.first != b.first || a.count != b.count || a.fp.hi != b.fp.hi || a.fp.lo != b.fp.lo || a.state != b.state)
      disagree++;
    printf("%s{\"first_depth\":%lld,\"holders\":%llu", w ? "," : "", a.first < 0 ? -1ll : in.depth0 + a.first, a.count);
    if (a.first >= 0) {
      printf(",\"hi\":\"%016llx\",\"lo\":\"%016llx\",\"trace_len\":%lld,\"state\":\"", (unsigned long long)a.fp.hi,
             (unsigned long long)a.fp.lo, a.first);
      for (uint32_t x : a.state)  // the packed state's bytes (little-endian words)
        printf("%02x%02x%02x%02x", x & 0xffu, (x >> 8) & 0xffu, (x >> 16) & 0xffu, x >> 24);
      printf("\"");
    }
    printf("}");
  }
  printf("],\"disagree\":%d,\"errors\":%d}\n", disagree, errors);
  return disagree || errors ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: witnesscheck <scenario> <blob>\n"), 2;
  Input in;
  if (!read_input(argv[2], &in)) return fprintf(stderr, "witnesscheck: bad blob\n"), 2;
  switch (in.desc.protocol) {
    case DSL_PROTO_PINGPONG: return witnesses<PingPong>(argv[1], in);
    case DSL_PROTO_MULTIPAXOS: return witnesses<MultiPaxos>(argv[1], in);
    case DSL_PROTO_PB: return witnesses<PB>(argv[1], in);
    case DSL_PROTO_PINGPONG_IR: return witnesses<PingPongIR>(argv[1], in);
    case DSL_PROTO_MULTIPAXOS_IR: return witnesses<MultiPaxosIR>(argv[1], in);
    case DSL_PROTO_PB_IR: return witnesses<PBIR>(argv[1], in);
    default: return fprintf(stderr, "witnesscheck: protocol %d is not wired in\n", in.desc.protocol), 2;
  }
}
