// tests/hostcheck/eventcheck.cpp -- TEST TOOL, not part of the product.
//
// The event census (dsl_set_event_census) on the host: a level-by-level BFS with exact state
// equality over the packed transition functions -- a map from the whole packed state to the depth
// at which it was first discovered; no fingerprint decides anything and there is no table. Under
// settings given as the engine receives them (resolve_settings, the engine's own path), for every
// (parent of the level, enabled event) with a non-null result:
//   * the cell (handler class, destination node) comes from the protocol's class functions:
//     P::msg_class / P::rec_to of the record, or Classes<P>::kTimer0 + TimerClasses<P>::of(node);
//   * an exceptional step counts as `exceptions` (and, as in the engine, as a new state);
//   * the successor is materialized; equal to its parent, byte for byte, it counts as `noops`;
//   * otherwise it is `fresh` when the map does not hold it at a depth <= the parent's: not at
//     all, or discovered earlier in this same level by another event.
// One JSON line: per_depth, the successors total, the rows as sparse cells [cls, to, events,
// noops, exceptions, fresh], and the terminal the search ended on (the level's candidate of the
// highest priority and the smallest fingerprint, as the engine reports it) for a next stage's start.
// Built also with -fsanitize=undefined.
//
// usage: eventcheck <scenario name> <blob>    blob: as tests/watch_cases.py writes it for watchcheck
//          (dsl_protocol_desc, dsl_settings, the watches -- ignored here --, the dropped records,
//          the start depth and state)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../dslabs_amd/csrc/protocols/all.hpp"
#include "../../dslabs_amd/csrc/settings.hpp"

using namespace dsl;

namespace {

struct Input {
  dsl_protocol_desc desc;
  dsl_settings hs;
  int32_t depth0 = 0;
  std::vector<uint64_t> dropped;
  std::vector<uint8_t> start;
};

bool read_input(const char* path, Input* in) {
  std::ifstream f(path, std::ios::binary);
  std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t o = 0;
  auto take = [&](void* dst, size_t n) {
    if (o + n > b.size()) return false;
    if (n && dst) std::memcpy(dst, b.data() + o, n);
    o += n;
    return true;
  };
  int32_t nw = 0, np = 0, nd = 0, nstart = 0, pad = 0;
  if (!take(&in->desc, sizeof(in->desc)) || !take(&in->hs, sizeof(in->hs)) || !take(&nw, 4) || !take(&np, 4) ||
      !take(nullptr, sizeof(dsl_predicate) * DSL_MAX_WATCHES) || !take(nullptr, sizeof(dsl_predicate) * DSL_MAX_POOL) ||
      !take(&nd, 4) || !take(&in->depth0, 4) || !take(&nstart, 4) || !take(&pad, 4) || nd < 0 || nstart < 0)
    return false;
  in->dropped.resize(nd);
  in->start.resize(nstart);
  return take(in->dropped.data(), 8 * (size_t)nd) && take(in->start.data(), (size_t)nstart) && o == b.size();
}

struct Cell {
  unsigned long long events = 0, noops = 0, exceptions = 0, fresh = 0;
};

template <class P>
int run(const char* name, const Input& in) {
  constexpr int NCLS = Classes<P>::kSkip;
  static_assert(NCLS <= DSL_EVENT_CLASSES && P::kNodes <= DSL_EVENT_NODES, "the ABI grid holds every cell");
  const typename P::Params prm = P::from_desc(in.desc);
  DevSettings set;
  std::string why;
  if (!P::valid(prm) || resolve_settings(in.hs, P::num_nodes(prm), &P::known_predicate, &set, &why) ||
      !check_field_leaves<P>(set, &why) || !check_net_leaves<P>(set, &why)) {
    fprintf(stderr, "settings refused: %s\n", why.c_str());
    return 1;
  }
  set_pred_reads<P>(set, prm);
  using S = typename P::State;
  using Rec = typename P::Rec;
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
  std::unordered_map<std::string, int> first{{key(init), in.depth0}};
  std::vector<unsigned long long> per_depth{1};
  std::vector<std::vector<Cell>> rows;
  unsigned long long successors = 0;
  int end = 0, pi = -1, term_depth = -1;
  // the terminal the engine reports: priority (exception > invariant > goal), then the fingerprint
  bool have_term = false;
  int best_v = 0;
  Fp best_fp{0, 0};
  S best_state{};
  auto candidate = [&](int v, const S& s) {
    const Fp f = full_fingerprint<P>(s.w);
    const bool better = !have_term || v < best_v ||
                        (v == best_v && ((f.hi >> 2) < (best_fp.hi >> 2) || ((f.hi >> 2) == (best_fp.hi >> 2) && f.lo < best_fp.lo)));
    if (better) best_v = v, best_fp = f, best_state = s, have_term = true;
  };
  std::vector<S> frontier;
  {
    const NodeView v0{init.w, P::kNodeWords, -1, nullptr};
    const int v = judge_view<P>(v0, prm, set, in.depth0, &pi);
    if (v >= V_TERM_EXCEPTION) end = v, term_depth = in.depth0;
    else frontier.push_back(init);  // the initial state is expanded also when pruned
  }
  for (int depth = in.depth0; !frontier.empty() && end == 0; depth++) {
    std::vector<Cell> row((size_t)NCLS * P::kNodes);
    std::vector<S> next;
    const size_t level = (size_t)(depth + 1 - in.depth0);
    auto discovered = [&] {
      if (per_depth.size() <= level) per_depth.resize(level + 1, 0);
      per_depth[level]++;
    };
    for (const S& par : frontier) {
      const int ne = count_events<P>(par.w, prm, set);
      for (int k = 0; k < ne; k++) {
        Delta<P> dl;
        const int rc = delta_step<P>(par.w, k, dl, prm, set);
        if (rc == STEP_NULL) continue;
        if (rc != STEP_OK && rc != STEP_EXCEPTION) {  // an overflow: the engine ends such a search with an error
          errors++;
          continue;
        }
        const int e = locate_event<P>(par.w, prm, set, k);
        int cls, to;
        if (e >= 0) {
          const Rec r = Net<P>::at(par.w, e);
          cls = P::msg_class(r);
          to = P::rec_to(r);
        } else {
          to = (-1 - e) >> 8;
          cls = Classes<P>::kTimer0 + TimerClasses<P>::of(to, prm);
        }
        if (cls < 0 || cls >= NCLS || to < 0 || to >= P::num_nodes(prm)) {
          errors++;
          continue;
        }
        Cell& c = row[(size_t)cls * P::kNodes + to];
        c.events++;
        successors++;
        if (rc == STEP_EXCEPTION) {  // equal to no other state: new, and terminal
          c.exceptions++;
          discovered();
          if (end == 0 || V_TERM_EXCEPTION < end) end = V_TERM_EXCEPTION;
          continue;
        }
        S t;
        if (!materialize<P>(par.w, dl, t.w)) {
          errors++;
          continue;
        }
        if (std::memcmp(t.w, par.w, sizeof(S)) == 0) {
          c.noops++;
          continue;
        }
        const auto ins = first.emplace(key(t), depth + 1);
        if (!ins.second) {
          if (ins.first->second == depth + 1) c.fresh++;  // discovered in this level by another event
          continue;
        }
        c.fresh++;
        discovered();
        NodeView view{par.w, P::kNodeWords, dl.node, dl.nw};
        Rec news[P::kMaxSends];
        view.sends = news;
        view.nsends = delta_sends<P>(dl, news);
        const int v = judge_view<P>(view, prm, set, depth + 1, &pi, depth > in.depth0);
        if (v >= V_TERM_EXCEPTION) {
          candidate(v, t);
          if (end == 0 || v < end) end = v;
          continue;
        }
        if (v == V_PRUNED) continue;
        next.push_back(t);
      }
    }
    rows.push_back(row);
    if (end) term_depth = depth + 1;
    frontier.swap(next);
  }
  printf("{\"scenario\":\"%s\",\"end\":%d,\"initial_depth\":%d,\"per_depth\":[", name, end, in.depth0);
  for (size_t i = 0; i < per_depth.size(); i++) printf("%s%llu", i ? "," : "", per_depth[i]);
  printf("],\"successors\":%llu,\"classes\":%d,\"nodes\":%d,\"rows\":[", successors, NCLS, P::num_nodes(prm));
  for (size_t i = 0; i < rows.size(); i++) {
    printf("%s[", i ? "," : "");
    bool firstc = true;
    for (int c = 0; c < NCLS; c++)
      for (int t = 0; t < P::kNodes; t++) {
        const Cell& x = rows[i][(size_t)c * P::kNodes + t];
        if (!x.events) continue;
        printf("%s[%d,%d,%llu,%llu,%llu,%llu]", firstc ? "" : ",", c, t, x.events, x.noops, x.exceptions, x.fresh);
        firstc = false;
      }
    printf("]");
  }
  printf("],\"terminal\":");
  if (have_term && best_v == end) {
    printf("{\"depth\":%d,\"state\":\"", term_depth);
    for (size_t i = 0; i < sizeof(S); i++) printf("%02x", ((const uint8_t*)best_state.w)[i]);
    printf("\"}");
  } else {
    printf("null");
  }
  printf(",\"errors\":%d}\n", errors);
  return errors ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: eventcheck <scenario> <blob>\n"), 2;
  Input in;
  if (!read_input(argv[2], &in)) return fprintf(stderr, "eventcheck: bad blob\n"), 2;
  switch (in.desc.protocol) {
    case DSL_PROTO_PINGPONG: return run<PingPong>(argv[1], in);
    case DSL_PROTO_SIPAXOS: return run<SIPaxos>(argv[1], in);
    case DSL_PROTO_MULTIPAXOS: return run<MultiPaxos>(argv[1], in);
    case DSL_PROTO_SYNTHETIC: return run<Synthetic>(argv[1], in);
    case DSL_PROTO_AMOKV: return run<AmoKV>(argv[1], in);
    case DSL_PROTO_PB: return run<PB>(argv[1], in);
    case DSL_PROTO_MINITEST: return run<MiniTest>(argv[1], in);
    case DSL_PROTO_PINGPONG_IR: return run<PingPongIR>(argv[1], in);
    case DSL_PROTO_AMOKV_IR: return run<AmoKVIR>(argv[1], in);
    case DSL_PROTO_MULTIPAXOS_IR: return run<MultiPaxosIR>(argv[1], in);
    case DSL_PROTO_PB_IR: return run<PBIR>(argv[1], in);
    default: return fprintf(stderr, "eventcheck: protocol %d is not wired in\n", in.desc.protocol), 2;
  }
}
