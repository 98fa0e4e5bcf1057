// tests/devcheck/emitcheck.hip -- TEST TOOL, not part of the product.
//
// The product's wave_emit (kernels.hpp) in isolation: one 64-lane wave per case writes the rows of
// crafted parents and deltas (tests/hostcheck/emit_cases.hpp) into a buffer pre-filled with a
// sentinel, in three modes -- parents in global memory (k_unspill's call), parents and the changed
// nodes' words in LDS (k_level's and k_materialize's, nw_lds), and the latter with the new-record
// mask returned (k_level with sleep sets). The host part restates every row with emit_row and
// creator_record (nodestate.hpp) and counts what differs; tests/test_gpu_emit.py judges the counts.
//
// usage: emitcheck <protocol id>
//
// One JSON object: "cases", each with name, mode, rows, header_bad, record_bad (a record below the
// count differs), sentinel_bad (a word past the count, of a row nobody owns, or of the guard rows
// around the buffer is not the sentinel), mask_bad, collision and expect_collision.
// Every HIP call is checked: the first error is printed and ends the program, non-zero, with
// nothing started after it.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../dslabs_amd/csrc/kernels.hpp"
#include "../hostcheck/emit_cases.hpp"

using namespace dsl;

namespace {

constexpr uint32_t kSentinel = 0xA5C3A5C3u;
constexpr uint64_t kMaskSentinel = 0xA5C3A5C3A5C3A5C3ull;

[[noreturn]] void die(const std::string& what) {
  fflush(stdout);
  fprintf(stderr, "emitcheck: %s\n", what.c_str());
  fflush(stderr);
  _exit(1);  // no destructors: nothing more touches the device
}

#define CHK(call)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      die(std::string("HIP error ") + hipGetErrorString(e_) + " at line " + std::to_string(__LINE__) + " (" #call ")"); \
  } while (0)

enum Mode : int { kGlobal = 0, kLds = 1, kLdsMask = 2 };

// Parents' rows are staged in LDS where 64 of them fit in 48 KB (every protocol but PingPongIR,
// whose rows then stay in global memory beside the LDS node words).
template <class P>
constexpr bool kStageRows = 64 * Layout<P>::kWords * 4 <= 48 * 1024;

// One wave: lane l owns parents[l] and deltas[l], active when bit l of `active`; its row goes to
// out + (1 + l) * NW (row 0 and row 65 are guards).
template <class P>
__global__ void __launch_bounds__(64) k_emit(const uint32_t* parents, const Delta<P>* deltas, uint64_t active,
                                             uint32_t* out, int mode, uint64_t* masks, uint32_t* coll) {
  constexpr int NW = Layout<P>::kWords;
  __shared__ uint32_t s_rows[kStageRows<P> ? 64 * NW : 1];
  __shared__ uint32_t s_nodew[64 * P::kNodeWords];
  const int lane = (int)threadIdx.x;
  const bool act = (active >> lane) & 1ull;
  Delta<P> d = deltas[lane];
  if constexpr (kStageRows<P>) {
    for (int o = lane; o < 64 * NW; o += 64) s_rows[o] = parents[o];
  }
  for (int i = 0; i < P::kNodeWords; i++) s_nodew[lane * P::kNodeWords + i] = d.nw[i];
  __syncthreads();
  uint32_t* dst = out + (size_t)(1 + lane) * NW;
  bool c;
  if (mode == kGlobal) {
    c = wave_emit<P>(act, parents, (uint64_t)lane, d, dst);
  } else {
    const uint32_t* base = kStageRows<P> ? s_rows : parents;
    if constexpr (MaskEmit<P>::value) {
      uint64_t m = kMaskSentinel;
      c = wave_emit<P>(act, base, (uint64_t)lane, d, dst, s_nodew, mode == kLdsMask ? &m : nullptr);
      masks[lane] = m;
    } else {
      c = wave_emit<P>(act, base, (uint64_t)lane, d, dst, s_nodew);
    }
  }
  if (lane == 0) *coll = c ? 1u : 0u;
}

template <class P>
struct WaveCase {
  std::string name;
  std::vector<emitcases::Case<P>> lanes;  // 64
  uint64_t active;
};

template <class P>
std::vector<WaveCase<P>> wave_cases() {
  std::vector<WaveCase<P>> out;
  auto filler = [](uint64_t seed) {
    std::vector<emitcases::Case<P>> v;
    for (int l = 0; l < 64; l++) v.push_back(emitcases::random_case<P>("lane" + std::to_string(l), seed * 64 + (uint64_t)l));
    return v;
  };
  int k = 0;
  for (const auto& c : emitcases::crafted<P>()) {  // each crafted row alone in its wave, in a lane of its own
    WaveCase<P> w{c.name, filler(1000 + (uint64_t)k), 0};
    const int lane = (k * 11 + 3) % 64;
    w.lanes[lane] = c;
    w.active = 1ull << lane;
    out.push_back(w);
    k++;
  }
  out.push_back({"active_none", filler(2001), 0ull});
  out.push_back({"active_lane0", filler(2002), 1ull});
  out.push_back({"active_lane63", filler(2003), 1ull << 63});
  out.push_back({"active_all64", filler(2004), ~0ull});
  out.push_back({"active_odd", filler(2005), 0xAAAAAAAAAAAAAAAAull});
  return out;
}

template <class P>
int run() {
  using L = Layout<P>;
  constexpr int NW = L::kWords;
  constexpr bool masked = MaskEmit<P>::value;
  hipStream_t st;
  CHK(hipSetDevice(0));
  CHK(hipStreamCreate(&st));
  uint32_t *d_par = nullptr, *d_out = nullptr, *d_coll = nullptr;
  Delta<P>* d_del = nullptr;
  uint64_t* d_masks = nullptr;
  const size_t out_words = (size_t)66 * NW;
  CHK(hipMalloc(&d_par, (size_t)64 * NW * 4));
  CHK(hipMalloc(&d_del, 64 * sizeof(Delta<P>)));
  CHK(hipMalloc(&d_out, out_words * 4));
  CHK(hipMalloc(&d_masks, 64 * 8));
  CHK(hipMalloc(&d_coll, 4));
  std::vector<uint32_t> par((size_t)64 * NW), got(out_words), fill(out_words, kSentinel);
  std::vector<Delta<P>> del(64);
  std::vector<uint64_t> masks(64), mfill(64, kMaskSentinel);
  printf("{\"masked\":%s,\"cases\":[", masked ? "true" : "false");
  bool first = true;
  for (const auto& wc : wave_cases<P>()) {
    for (int l = 0; l < 64; l++) {
      for (int o = 0; o < NW; o++) par[(size_t)l * NW + o] = wc.lanes[l].pw[o];
      del[l] = wc.lanes[l].d;
    }
    CHK(hipMemcpyAsync(d_par, par.data(), par.size() * 4, hipMemcpyHostToDevice, st));
    CHK(hipMemcpyAsync(d_del, del.data(), 64 * sizeof(Delta<P>), hipMemcpyHostToDevice, st));
    for (int mode = kGlobal; mode <= kLdsMask; mode++) {
      if (mode == kLdsMask && !masked) continue;
      uint32_t coll = 0xffffffffu;
      CHK(hipMemcpyAsync(d_out, fill.data(), out_words * 4, hipMemcpyHostToDevice, st));
      CHK(hipMemcpyAsync(d_masks, mfill.data(), 64 * 8, hipMemcpyHostToDevice, st));
      CHK(hipMemcpyAsync(d_coll, &coll, 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_emit<P>, dim3(1), dim3(64), 0, st, d_par, d_del, wc.active, d_out, mode, d_masks, d_coll);
      CHK(hipGetLastError());
      CHK(hipStreamSynchronize(st));
      CHK(hipMemcpy(got.data(), d_out, out_words * 4, hipMemcpyDeviceToHost));
      CHK(hipMemcpy(masks.data(), d_masks, 64 * 8, hipMemcpyDeviceToHost));
      CHK(hipMemcpy(&coll, d_coll, 4, hipMemcpyDeviceToHost));
      long long rows = 0, header_bad = 0, record_bad = 0, sentinel_bad = 0, mask_bad = 0;
      bool expect = false;
      for (int o = 0; o < NW; o++) sentinel_bad += (got[o] != kSentinel) + (got[(size_t)65 * NW + o] != kSentinel);
      for (int l = 0; l < 64; l++) {
        const uint32_t* g = got.data() + (size_t)(1 + l) * NW;
        const auto& c = wc.lanes[l];
        if (!((wc.active >> l) & 1ull)) {
          for (int o = 0; o < NW; o++) sentinel_bad += g[o] != kSentinel;
          if (mode == kLdsMask) mask_bad += masks[l] != kMaskSentinel;
          continue;
        }
        rows++;
        if (c.equal_sends) {  // reported by the protocols whose emitter looks (see wave_emit); no row is defined
          expect = expect || masked || SendsDistinct<P>::value;
          continue;
        }
        uint32_t want[NW];
        if (!emit_row<P>(c.pw, c.d, want)) die("a case that overflows the network");
        for (int o = 0; o < L::kRecBase; o++) header_bad += g[o] != want[o];
        const int cnt = Net<P>::size(want);
        for (int q = 0; q < cnt; q++) record_bad += Net<P>::at(g, q) != Net<P>::at(want, q);
        for (int o = L::kRecBase + cnt * L::kRecWords; o < NW; o++) sentinel_bad += g[o] != kSentinel;
        if (mode == kLdsMask) {
          uint32_t cw;
          uint64_t cm;
          creator_record<P>(c.pw, -1, c.d, &cw, &cm);
          mask_bad += masks[l] != cm;
        }
      }
      printf("%s{\"name\":\"%s\",\"mode\":%d,\"rows\":%lld,\"header_bad\":%lld,\"record_bad\":%lld,\"sentinel_bad\":%lld,"
             "\"mask_bad\":%lld,\"collision\":%u,\"expect_collision\":%d}",
             first ? "" : ",", wc.name.c_str(), mode, rows, header_bad, record_bad, sentinel_bad, mask_bad, coll,
             expect ? 1 : 0);
      first = false;
    }
  }
  printf("]}\n");
  fflush(stdout);
  _exit(0);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: emitcheck <protocol id>");
  switch (atoi(argv[1])) {
    case DSL_PROTO_SIPAXOS: return run<SIPaxos>();
    case DSL_PROTO_MULTIPAXOS: return run<MultiPaxos>();
    case DSL_PROTO_PB: return run<PB>();
    case DSL_PROTO_MINITEST: return run<MiniTest>();
    case DSL_PROTO_PINGPONG_IR: return run<PingPongIR>();
  }
  die("unknown protocol");
}
