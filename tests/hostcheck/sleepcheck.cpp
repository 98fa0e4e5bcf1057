// tests/hostcheck/sleepcheck.cpp -- TEST TOOL, not part of the product.
//
// The sleep-set rule (dslabs_amd/csrc/nodestate.hpp: creator_record, sleeping, sleep_sets_apply)
// on the host: a level-synchronous BFS with exact state equality over the packed transition
// functions, which keeps each frontier state's recorded parent row and so checks what the device
// cannot.
//   1. Race independence: when several (parent, event) pairs generate a state in one level, the
//      recorded creator is picked at random among them (seeded). Every seed's per-depth counts,
//      state count, successor count and end (level, verdict, predicate) must equal the plain BFS.
//   2. The commuting property, for every sleeping event E of a state P with recorded parent G and
//      creator Cr: E's record is in G's network ("not_enabled"), its handler gives the same node
//      words and sends at G ("delta_differs"), and G+E+Cr has the fingerprint of P+E ("fp_differs").
//   3. The new-record mask marks exactly the records of the successor that its parent lacks
//      ("mask_mismatch").
//   4. "rule_on" tells whether the settings allowed the rule (sleep_sets_apply): never with a
//      prune or a dropped link; then no event sleeps.
//
// usage: sleepcheck <blob> <seeds>     blob = dsl_protocol_desc + dsl_settings (tools/cpu_baseline.py)
// prints one JSON line.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../dslabs_amd/csrc/protocols/all.hpp"
#include "../../dslabs_amd/csrc/settings.hpp"

using namespace dsl;

namespace {

struct Outcome {
  std::vector<unsigned long long> per_depth;
  unsigned long long states = 0, successors = 0, slept = 0, slept_unfiltered = 0;
  int end_level = -1, verdict = 99, pred = -1;
  bool operator==(const Outcome& o) const {
    return per_depth == o.per_depth && states == o.states && successors == o.successors && end_level == o.end_level &&
           verdict == o.verdict && pred == o.pred;
  }
};

struct Faults {
  unsigned long long not_enabled = 0, delta_differs = 0, fp_differs = 0, mask_mismatch = 0, errors = 0;
};

uint64_t next_rand(uint64_t& s) {  // splitmix64
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

template <class P>
struct Front {
  typename P::State s;
  typename P::State g;  // the recorded parent's row
  int cr = INT32_MIN;   // the creator's located event in g
  uint32_t cw = 0;      // the creator record (0: none)
  uint64_t cm = 0;
};

template <class P>
Outcome bfs(const typename P::Params& prm, const DevSettings& set, bool rule, uint64_t seed, Faults& ft) {
  using S = typename P::State;
  using Rec = typename P::Rec;
  auto key = [](const S& s) { return std::string((const char*)s.w, sizeof(S)); };
  Outcome o;
  S init;
  if (!init_state<P>(init.w, prm)) {
    ft.errors++;
    return o;
  }
  std::unordered_set<std::string> seen{key(init)};
  o.per_depth.assign(1, 1);
  o.states = 1;
  std::vector<Front<P>> cur(1), nxt;
  cur[0].s = init;
  {
    int pi = -1;
    const NodeView v0{init.w, P::kNodeWords, -1, nullptr};
    const int v = judge_view<P>(v0, prm, set, 0, &pi);
    if (v >= V_TERM_EXCEPTION) {
      o.end_level = 0;
      o.verdict = v;
      o.pred = pi;
      return o;
    }
  }
  struct Cand {
    size_t parent;
    int e;
    uint32_t cw;
    uint64_t cm;
    S x;
  };
  for (int depth = 0; !cur.empty() && o.verdict == 99; depth++) {
    std::unordered_map<std::string, std::vector<Cand>> gen;  // this level's new states and their generators
    std::vector<std::string> order;                          // ... in first-generation order
    for (size_t p = 0; p < cur.size(); p++) {
      const Front<P>& f = cur[p];
      const uint32_t* w = f.s.w;
      const int ne = count_events<P>(w, prm, set);
      for (int k = 0; k < ne; k++) {
        const int e = locate_event<P>(w, prm, set, k);
        if (rule && e >= 0 && sleeping<P>(w, f.cw, f.cm, e, prm)) {
          o.slept++;
          o.successors++;
          const Rec r = Net<P>::at(w, e);
          if (!NoopFilter<P>::msg(P::rec_to(r), w, r, prm)) o.slept_unfiltered++;
          // the commuting property against the recorded parent
          int ge = -1;
          for (int j = 0; j < Net<P>::size(f.g.w); j++)
            if (Net<P>::at(f.g.w, j) == r) ge = j;
          if (ge < 0 || locate_event<P>(f.g.w, prm, set, ge) != ge) {
            ft.not_enabled++;
            continue;
          }
          Delta<P> dp, dg;
          const int rp = delta_step_located<P>(w, e, dp, prm, set), rg = delta_step_located<P>(f.g.w, ge, dg, prm, set);
          bool same = rp == rg && dp.node == dg.node && dp.out.n == dg.out.n &&
                      same_words<P::kNodeWords>(dp.nw, dg.nw);
          for (int i = 0; same && i < dp.out.n; i++) same = dp.out.r[i] == dg.out.r[i];
          if (!same || rp != STEP_OK) {
            ft.delta_differs++;
            continue;
          }
          S pe, ge_s, x;
          if (!materialize<P>(w, dp, pe.w) || !materialize<P>(f.g.w, dg, ge_s.w)) {
            ft.errors++;
            continue;
          }
          int cr = f.cr;  // a timer keeps its code (its node is unchanged); a message is found by value
          if (f.cr >= 0) {
            const Rec crr = Net<P>::at(f.g.w, f.cr);
            cr = INT32_MIN;
            for (int j = 0; j < Net<P>::size(ge_s.w); j++)
              if (Net<P>::at(ge_s.w, j) == crr) cr = j;
          }
          Delta<P> dc;
          if (cr == INT32_MIN || delta_step_located<P>(ge_s.w, cr, dc, prm, set) != STEP_OK || !materialize<P>(ge_s.w, dc, x.w)) {
            ft.fp_differs++;
            continue;
          }
          const Fp a = full_fingerprint<P>(x.w), b = full_fingerprint<P>(pe.w);
          if (a.hi != b.hi || a.lo != b.lo || key(x) != key(pe)) ft.fp_differs++;
          continue;
        }
        Delta<P> d;
        const int rc = delta_step_located<P>(w, e, d, prm, set);
        if (rc == STEP_NULL) continue;
        o.successors++;
        if (rc == STEP_EXCEPTION) {  // never equal to another state: new and terminal
          if (o.per_depth.size() <= (size_t)depth + 1) o.per_depth.resize(depth + 2, 0);
          o.per_depth[depth + 1]++;
          o.states++;
          o.end_level = depth + 1;
          o.verdict = std::min(o.verdict, (int)V_TERM_EXCEPTION);
          continue;
        }
        if (rc != STEP_OK) {
          ft.errors++;
          continue;
        }
        Cand c;
        c.parent = p;
        c.e = e;
        if (!materialize<P>(w, d, c.x.w)) {
          ft.errors++;
          continue;
        }
        const std::string kx = key(c.x);
        if (seen.count(kx)) continue;
        creator_record<P>(w, e, d, &c.cw, &c.cm);
        if (SleepSets<P>::value) {  // the mask against the materialized row
          uint64_t want = 0;
          for (int j = 0; j < Net<P>::size(c.x.w); j++)
            if (!Net<P>::contains(w, Net<P>::at(c.x.w, j))) want |= 1ull << (j & 63);
          if (want != c.cm) ft.mask_mismatch++;
        }
        auto it = gen.find(kx);
        if (it == gen.end()) {
          order.push_back(kx);
          it = gen.emplace(kx, std::vector<Cand>()).first;
        }
        it->second.push_back(c);
      }
    }
    // the level's new states: judged once each, their creator drawn among their generators
    nxt.clear();
    uint64_t best_key = ~0ull;
    for (const std::string& kx : order) {
      const std::vector<Cand>& cs = gen[kx];
      const Cand& c = cs[(size_t)(next_rand(seed) % cs.size())];
      seen.insert(kx);
      if (o.per_depth.size() <= (size_t)depth + 1) o.per_depth.resize(depth + 2, 0);
      o.per_depth[depth + 1]++;
      o.states++;
      int pi = -1;
      const NodeView v{c.x.w, P::kNodeWords, -1, nullptr};
      const int verdict = judge_view<P>(v, prm, set, depth + 1, &pi);
      if (verdict >= V_TERM_EXCEPTION) {  // the level's best: by priority, then by fingerprint
        const uint64_t tk = ((uint64_t)(verdict - V_TERM_EXCEPTION) << 62) | (full_fingerprint<P>(c.x.w).hi >> 2);
        if (tk < best_key && o.verdict != V_TERM_EXCEPTION) {
          best_key = tk;
          o.verdict = verdict;
          o.pred = pi;
          o.end_level = depth + 1;
        }
        continue;
      }
      if (verdict != V_VALID) continue;
      Front<P> n;
      n.s = c.x;
      n.g = cur[c.parent].s;
      n.cr = c.e;
      n.cw = c.cw;
      n.cm = c.cm;
      nxt.push_back(n);
    }
    cur.swap(nxt);
  }
  return o;
}

void print_outcome(const char* name, const Outcome& o) {
  printf("\"%s\":{\"states\":%llu,\"successors\":%llu,\"end_level\":%d,\"verdict\":%d,\"pred\":%d,\"slept\":%llu,"
         "\"slept_unfiltered\":%llu,\"per_depth\":[",
         name, o.states, o.successors, o.end_level, o.verdict == 99 ? 0 : o.verdict, o.pred, o.slept, o.slept_unfiltered);
  for (size_t i = 0; i < o.per_depth.size(); i++) printf("%s%llu", i ? "," : "", o.per_depth[i]);
  printf("]}");
}

template <class P>
int run(const dsl_protocol_desc& d, const dsl_settings& hs, int seeds) {
  const typename P::Params prm = P::from_desc(d);
  if (!P::valid(prm)) return fprintf(stderr, "invalid params\n"), 2;
  DevSettings set;
  std::string why;
  if (resolve_settings(hs, P::num_nodes(prm), &P::known_predicate, &set, &why) || !check_field_leaves<P>(set, &why) ||
      !check_net_leaves<P>(set, &why))
    return fprintf(stderr, "settings: %s\n", why.c_str()), 2;
  set_pred_reads<P>(set, prm);
  const bool rule = sleep_sets_apply<P>(set);
  Faults ft;
  const Outcome plain = bfs<P>(prm, set, false, 1, ft);
  int differing = 0;
  Outcome last = plain;
  unsigned long long slept = 0;
  for (int s = 0; s < seeds; s++) {
    const Outcome o = bfs<P>(prm, set, rule, 0x5EED0000ull + (uint64_t)s, ft);
    differing += !(o == plain);
    slept += o.slept;
    last = o;
  }
  printf("{\"rule_on\":%s,\"seeds\":%d,\"differing\":%d,\"slept_all_seeds\":%llu,\"not_enabled\":%llu,"
         "\"delta_differs\":%llu,\"fp_differs\":%llu,\"mask_mismatch\":%llu,\"errors\":%llu,",
         rule ? "true" : "false", seeds, differing, slept, ft.not_enabled, ft.delta_differs, ft.fp_differs,
         ft.mask_mismatch, ft.errors);
  print_outcome("plain", plain);
  printf(",");
  print_outcome("last", last);
  printf("}\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return fprintf(stderr, "usage: sleepcheck <blob> <seeds>\n"), 2;
  dsl_protocol_desc d;
  dsl_settings s;
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(&d, sizeof d, 1, f) != 1 || fread(&s, sizeof s, 1, f) != 1)
    return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  fclose(f);
  const int seeds = std::max(1, atoi(argv[2]));
  switch (d.protocol) {
    case DSL_PROTO_PINGPONG: return run<PingPong>(d, s, seeds);
    case DSL_PROTO_SIPAXOS: return run<SIPaxos>(d, s, seeds);
    case DSL_PROTO_MULTIPAXOS: return run<MultiPaxos>(d, s, seeds);
    case DSL_PROTO_SYNTHETIC: return run<Synthetic>(d, s, seeds);
    case DSL_PROTO_AMOKV: return run<AmoKV>(d, s, seeds);
    case DSL_PROTO_PB: return run<PB>(d, s, seeds);
    case DSL_PROTO_MINITEST: return run<MiniTest>(d, s, seeds);
  }
  return fprintf(stderr, "unknown protocol\n"), 2;
}
