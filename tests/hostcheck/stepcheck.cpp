// tests/hostcheck/stepcheck.cpp -- TEST TOOL, not part of the product.
//
// Step invariants (dsl_set_step_invariants) on the host: a level-by-level BFS with exact state
// equality over the packed transition functions -- a map from the whole packed state to the depth
// at which it was first discovered; no fingerprint decides identity and there is no table. Under
// settings and step invariants given as the engine receives them (resolve_settings, the engine's
// own path), every judged edge -- (parent of the level, enabled event) whose handler returns
// STEP_OK and whose materialized successor differs from its parent, byte for byte -- has each step
// invariant evaluated TWICE:
//   * through eval_step_prog on the delta view (the product's function, with delta_step_hits);
//   * by plain C++ over the dsl_predicate tree as the caller wrote it, on the two materialized
//     states, the list of records the successor has and the parent lacks, and the event's class
//     and node from the protocol's class functions.
// Any difference between the two is an error (non-zero exit). The search ends at the first level
// with a violated edge (after the level), or as the plain search ends; the reported edge is the
// violating one with the smallest (parent fingerprint hi, lo, event index) -- the product's
// fingerprint function is the definition of that order.
// One JSON line: per_depth, the edge rows, the end, the violation (index, depth, parent and
// successor bytes, event, counts) and three diagnostics of the violating level: its violating
// edges, the successors reached by both a violating and a non-violating edge, and the violating
// edges that lead to a state first discovered at a shallower depth.
// Built also with -fsanitize=undefined.
//
// usage: stepcheck <scenario name> <blob>    blob: as tests/step_cases.py writes it
//          (tests/watch_cases.py's blob -- the watches are ignored here -- then the step
//          invariants: n, n_pool, 8 + 48 dsl_predicate)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <tuple>
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
  int32_t n_step = 0, n_spool = 0;
  dsl_predicate step[DSL_MAX_STEP_INVARIANTS];
  dsl_predicate spool[DSL_MAX_POOL];
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
  if (!take(in->dropped.data(), 8 * (size_t)nd) || !take(in->start.data(), (size_t)nstart)) return false;
  return take(&in->n_step, 4) && take(&in->n_spool, 4) && take(in->step, sizeof(in->step)) &&
         take(in->spool, sizeof(in->spool)) && o == b.size() && in->n_step >= 0 &&
         in->n_step <= DSL_MAX_STEP_INVARIANTS && in->n_spool >= 0 && in->n_spool <= DSL_MAX_POOL;
}

bool cmp_holds(int cmp, uint64_t a, uint64_t b) {
  switch (cmp) {
    case DSL_CMP_EQ: return a == b;
    case DSL_CMP_NE: return a != b;
    case DSL_CMP_LT: return a < b;
    case DSL_CMP_GE: return a >= b;
    case DSL_CMP_LE: return a <= b;
    default: return a > b;
  }
}

// The second evaluation: the caller's tree, the two whole states, plain arithmetic.
template <class P>
struct Plain {
  using S = typename P::State;
  using Rec = typename P::Rec;
  const Input& in;
  const typename P::Params& prm;
  const DevSettings& set;
  const S* par;
  const S* succ;
  std::vector<Rec> added;
  int cls = -1, to = -1;

  static uint64_t field(const S& s, uint32_t desc) {
    const int node = DSL_FIELD_NODE(desc), bit = DSL_FIELD_BIT(desc), width = DSL_FIELD_WIDTH(desc);
    const uint64_t word = s.w[node * P::kNodeWords + bit / 32];
    return (word >> (bit % 32)) & ((1ull << width) - 1ull);
  }
  int leaf(const dsl_predicate& p) const {
    if (p.pred_id == DSL_PRED_STEP_FIELD || p.pred_id == DSL_PRED_FIELD) {
      const bool stepf = p.pred_id == DSL_PRED_STEP_FIELD;
      const S& ls = stepf && !DSL_STEP_ARG0_LHS_NEW(p.arg0) ? *par : *succ;
      const S& rs = stepf && !DSL_STEP_ARG0_RHS_NEW(p.arg0) ? *par : *succ;
      const uint64_t a = field(ls, DSL_FIELD_ARG0_DESC(p.arg0));
      const uint64_t b = DSL_FIELD_ARG0_RHS_IS_FIELD(p.arg0) ? field(rs, (uint32_t)p.arg1) : (uint64_t)p.arg1;
      return cmp_holds(DSL_FIELD_ARG0_CMP(p.arg0), a, b) ? PV_TRUE : PV_FALSE;
    }
    if (p.pred_id == DSL_PRED_STEP_SENT) {
      for (Rec r : added) {
        bool all = true;
        for (int c = 0; c < (int)p.arg1; c++) {
          const dsl_predicate& q = in.spool[p.arg0 + c];
          const int bit = DSL_REC_ARG0_BIT(q.arg0), width = DSL_REC_ARG0_WIDTH(q.arg0);
          const uint64_t x = ((uint64_t)r >> bit) & ((1ull << width) - 1ull);
          all = all && cmp_holds(DSL_REC_ARG0_CMP(q.arg0), x, (uint64_t)q.arg1);
        }
        if (all) return PV_TRUE;
      }
      return PV_FALSE;
    }
    if (p.pred_id == DSL_PRED_STEP_EVENT)
      return (p.arg0 < 0 || p.arg0 == cls) && (p.arg1 < 0 || p.arg1 == to) ? PV_TRUE : PV_FALSE;
    // a named leaf of the protocol, on the whole successor
    DevPred op{p.pred_id, 0, (int32_t)p.arg0, (int32_t)p.arg1, 0u, 0u};
    op.reads = P::pred_reads(op, prm);
    NodeView v{succ->w, P::kNodeWords, -1, nullptr};
    v.dropped = set.dropped();
    v.ndropped = set.n_dropped;
    return P::eval(op, v, prm);
  }
  int eval(const dsl_predicate& p) const {
    int x;
    if (p.pred_id == DSL_PRED_AND || p.pred_id == DSL_PRED_OR || p.pred_id == DSL_PRED_IMPLIES) {
      int a = eval(in.spool[p.arg0]);
      if (p.pred_id == DSL_PRED_IMPLIES && a != PV_THREW) a = !a;  // or(negate(a), b)
      if (a == PV_THREW) x = PV_THREW;
      else if (p.pred_id == DSL_PRED_AND) x = a == PV_FALSE ? PV_FALSE : eval(in.spool[p.arg1]);
      else x = a == PV_TRUE ? PV_TRUE : eval(in.spool[p.arg1]);
    } else {
      x = leaf(p);
    }
    if (x != PV_THREW && p.negate) x = !x;
    return x;
  }
};

template <class S>
void print_hex(const S& s) {
  for (size_t i = 0; i < sizeof(S); i++) printf("%02x", ((const uint8_t*)s.w)[i]);
}

template <class P>
int run(const char* name, const Input& in) {
  const typename P::Params prm = P::from_desc(in.desc);
  DevSettings set;
  DevStep step;
  std::string why;
  const StepList sl{in.step, in.n_step, in.spool, in.n_spool};
  if (!P::valid(prm) || resolve_settings(in.hs, P::num_nodes(prm), &P::known_predicate, &set, &why, nullptr, &sl, &step) ||
      !check_field_leaves<P>(set, &why) || !check_net_leaves<P>(set, &why) || !check_step_leaves<P>(set, step, prm, &why)) {
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
  int errors = 0, mismatches = 0;
  if (!init_state<P>(init.w, prm)) return 1;
  if (!in.start.empty()) {
    if (in.start.size() != sizeof(S)) return 1;
    std::memcpy(init.w, in.start.data(), sizeof(S));
  }
  auto key = [](const S& s) { return std::string((const char*)s.w, sizeof(S)); };
  std::unordered_map<std::string, int> first{{key(init), in.depth0}};
  std::vector<unsigned long long> per_depth{1}, edges;
  int end = 0, term_depth = -1;
  // the terminal the plain search reports: priority (exception > invariant > goal), then the fingerprint
  bool have_term = false;
  int best_v = 0, best_pi = -1;
  Fp best_fp{0, 0};
  auto candidate = [&](int v, int pi, const S& s) {
    const Fp f = full_fingerprint<P>(s.w);
    const bool better = !have_term || v < best_v ||
                        (v == best_v && ((f.hi >> 2) < (best_fp.hi >> 2) || ((f.hi >> 2) == (best_fp.hi >> 2) && f.lo < best_fp.lo)));
    if (better) best_v = v, best_pi = pi, best_fp = f, have_term = true;
  };
  // the violation: the level's violating edge with the smallest (parent fp hi, lo, event)
  bool viol_found = false;
  std::tuple<uint64_t, uint64_t, int> viol_key;
  S viol_par{}, viol_succ{};
  int viol_index = -1, viol_k = -1, viol_depth = -1;
  unsigned long long viol_edges = 0, per_inv[DSL_MAX_STEP_INVARIANTS] = {}, both = 0, shallower = 0;
  std::vector<S> frontier;
  {
    int pi = -1;
    const NodeView v0{init.w, P::kNodeWords, -1, nullptr};
    const int v = judge_view<P>(v0, prm, set, in.depth0, &pi);
    if (v >= V_TERM_EXCEPTION) end = v, term_depth = in.depth0, best_v = v, best_pi = pi, have_term = v != V_TERM_EXCEPTION;
    else frontier.push_back(init);  // the initial state is expanded also when pruned
  }
  Plain<P> plain{in, prm, set, nullptr, nullptr, {}, -1, -1};
  for (int depth = in.depth0; !frontier.empty() && end == 0 && !viol_found; depth++) {
    std::vector<S> next;
    const size_t level = (size_t)(depth + 1 - in.depth0);
    unsigned long long judged = 0;
    std::unordered_map<std::string, int> reach;  // successor -> 1: by a violating edge, 2: by a non-violating one
    auto discovered = [&] {
      if (per_depth.size() <= level) per_depth.resize(level + 1, 0);
      per_depth[level]++;
    };
    for (const S& par : frontier) {
      const int ne = count_events<P>(par.w, prm, set);
      const Fp pf = full_fingerprint<P>(par.w);
      for (int k = 0; k < ne; k++) {
        Delta<P> dl;
        const int rc = delta_step<P>(par.w, k, dl, prm, set);
        if (rc == STEP_NULL) continue;
        if (rc != STEP_OK && rc != STEP_EXCEPTION) {  // an overflow: the engine ends such a search with an error
          errors++;
          continue;
        }
        if (rc == STEP_EXCEPTION) {  // no successor: not judged; new, and terminal
          discovered();
          if (end == 0 || V_TERM_EXCEPTION < end) end = V_TERM_EXCEPTION;
          continue;
        }
        S t;
        if (!materialize<P>(par.w, dl, t.w)) {
          errors++;
          continue;
        }
        if (std::memcmp(t.w, par.w, sizeof(S)) == 0) continue;  // a stuttering step: exempt
        // ---- the edge is judged, whatever becomes of its successor ----
        judged++;
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
        NodeView view{par.w, P::kNodeWords, dl.node, dl.nw};
        Rec news[P::kMaxSends];
        view.sends = news;
        view.nsends = delta_sends<P>(dl, news);
        const uint32_t hits = delta_step_hits<P>(set, step, dl);
        int c2 = -1, t2 = -1;
        if (step.has_event) step_event_cell<P>(par.w, e, prm, &c2, &t2);
        plain.par = &par;
        plain.succ = &t;
        plain.cls = cls;
        plain.to = to;
        plain.added.clear();
        for (int j = 0; j < Net<P>::size(t.w); j++)
          if (!Net<P>::contains(par.w, Net<P>::at(t.w, j))) plain.added.push_back(Net<P>::at(t.w, j));
        uint32_t viol = 0;
        for (int s = 0; s < step.n_step; s++) {
          const int a = eval_step_prog<P>(set, step.prog[s], view, prm, hits, c2, t2);
          const int b = plain.eval(in.step[s]);
          if (a != b) {
            if (mismatches++ < 5)
              fprintf(stderr, "MISMATCH depth %d event %d step invariant %d: eval_step_prog %d, plain %d\n", depth, k, s, a, b);
          }
          if (b != PV_TRUE) viol |= 1u << s;
        }
        int& rf = reach[key(t)];
        rf |= viol ? 1 : 2;
        if (viol) {
          viol_edges++;
          for (int s = 0; s < step.n_step; s++) per_inv[s] += (viol >> s) & 1u;
          const auto kk = std::make_tuple(pf.hi, pf.lo, k);
          if (viol_index < 0 || kk < viol_key) {
            viol_key = kk;
            viol_par = par;
            viol_succ = t;
            viol_index = __builtin_ctz(viol);
            viol_k = k;
            viol_depth = depth + 1;
          }
        }
        // ---- the plain search ----
        const auto ins = first.emplace(key(t), depth + 1);
        if (viol && ins.first->second < depth + 1) shallower++;
        if (!ins.second) continue;
        discovered();
        int pi = -1;
        const int v = judge_view<P>(view, prm, set, depth + 1, &pi, depth > in.depth0);
        if (v >= V_TERM_EXCEPTION) {
          candidate(v, pi, t);
          if (end == 0 || v < end) end = v;
          continue;
        }
        if (v == V_PRUNED) continue;
        next.push_back(t);
      }
    }
    edges.push_back(judged);
    if (viol_index >= 0) {
      viol_found = true;
      for (const auto& kv : reach) both += kv.second == 3;
    }
    if (end) term_depth = depth + 1;
    frontier.swap(next);
  }
  // the end: EXCEPTION > state INVARIANT > step INVARIANT > GOAL
  int end_condition, pred_index = -1, terminal_depth = term_depth;
  const bool step_wins = viol_found && !(end == V_TERM_EXCEPTION || end == V_TERM_INVARIANT);
  if (step_wins) {
    end_condition = DSL_INVARIANT_VIOLATED;
    pred_index = in.hs.n_invariants + viol_index;
    terminal_depth = viol_depth;
  } else if (end) {
    end_condition = end == V_TERM_EXCEPTION ? DSL_EXCEPTION_THROWN : end == V_TERM_INVARIANT ? DSL_INVARIANT_VIOLATED : DSL_GOAL_FOUND;
    pred_index = end == V_TERM_EXCEPTION ? -1 : best_pi;
  } else {
    end_condition = DSL_SPACE_EXHAUSTED;
  }
  printf("{\"scenario\":\"%s\",\"end\":%d,\"pred_index\":%d,\"terminal_depth\":%d,\"step_terminal\":%s,\"initial_depth\":%d,"
         "\"per_depth\":[", name, end_condition, pred_index, terminal_depth, step_wins ? "true" : "false", in.depth0);
  for (size_t i = 0; i < per_depth.size(); i++) printf("%s%llu", i ? "," : "", per_depth[i]);
  printf("],\"edges\":[");
  for (size_t i = 0; i < edges.size(); i++) printf("%s%llu", i ? "," : "", edges[i]);
  printf("],\"violation\":");
  if (viol_found) {
    dsl_event ev;
    describe_event<P>(viol_par.w, viol_k, prm, set, &ev);
    printf("{\"index\":%d,\"depth\":%d,\"parent\":\"", viol_index, viol_depth);
    print_hex(viol_par);
    printf("\",\"state\":\"");
    print_hex(viol_succ);
    printf("\",\"event\":{\"k\":%d,\"is_timer\":%d,\"from\":%d,\"to\":%d,\"type\":%d,\"fields\":[", viol_k, ev.is_timer, ev.from,
           ev.to, ev.type);
    for (int i = 0; i < ev.n_fields; i++) printf("%s%lld", i ? "," : "", (long long)ev.fields[i]);
    printf("]},\"edges\":%llu,\"per_invariant\":[", viol_edges);
    for (int s = 0; s < step.n_step; s++) printf("%s%llu", s ? "," : "", per_inv[s]);
    printf("],\"both\":%llu,\"shallower\":%llu}", both, shallower);
  } else {
    printf("null");
  }
  printf(",\"mismatches\":%d,\"errors\":%d}\n", mismatches, errors);
  return errors || mismatches ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: stepcheck <scenario> <blob>\n"), 2;
  Input in;
  if (!read_input(argv[2], &in)) return fprintf(stderr, "stepcheck: bad blob\n"), 2;
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
    default: return fprintf(stderr, "stepcheck: protocol %d is not wired in\n", in.desc.protocol), 2;
  }
}
