// tests/devcheck/tablecheck.hip -- TEST TOOL, not part of the product.
//
// The visited table's kernels (k_probe_remote, k_probe_slab, k_rehash, k_route_headers,
// k_new_list) and its layout functions (table_key0, table_home, table_rehome) run in isolation:
// the product's own, from kernels.hpp; this file holds no copy of either. It reads a scenario,
// executes its operations in order on one stream and prints what they left as one JSON object
// {"results": [...]}, one entry per operation. It judges nothing: tests/tablecheck_util.py makes
// the scenarios, tests/table_model.py is the reference.
//
// usage: tablecheck <scenario file>
//
// The scenario is little-endian 64-bit words: kMagic, then operations (a code, then its
// arguments; images of 32-bit words or bytes are padded to a whole word):
//   1 table b b0 load_first                a zeroed table of 2^b buckets
//   2 probe_remote n, n x (hi, lo)         k_probe_remote over the n records
//   3 slab_load W me cs, out_key in_key out_pk in_pk
//                                          the routed regions of shard `me` as the engine holds
//                                          them: what it routed (out_*: W regions, its own among
//                                          them) and what it received (in_*: one region per source)
//   4 probe_slab packed reply              k_probe_slab over them; reply 0 = the maxDepth level
//   5 rehash b2                            k_rehash into a zeroed table of 2^b2 buckets
//   6 route_headers received pk zero, W x kRouteSegs counters
//                                          k_route_headers into the out_* regions (received = 1:
//                                          into the in_* regions, as a source's that was sent)
//   7 new_list dev W cap cs, counters (dev: W x kRouteSegs, else kMaxShards), W x cap reply bytes
//                                          k_new_list with device counts or the host's
//   8 dump                                 every slot word
//   9 layout n, n x (b0 b b2 hi lo i v)    no GPU call: table_key0 and table_home of (hi, lo) in
//                                          a table of 2^b buckets, table_rehome of word v at slot
//                                          i of that table into one of 2^b2 buckets
// Replies are pre-filled with 0xAA, lists with ~0. Grids are the engine's (bfs_engine.hpp).
// Every HIP call is checked: the first error is printed and ends the program, non-zero, with
// nothing started after it.
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../dslabs_amd/csrc/kernels.hpp"

using namespace dsl;

namespace {

constexpr uint64_t kMagic = 0x31304b48434c4254ull;  // "TBLCHK01"
constexpr int kMaxLog2Buckets = 22;                 // 256 MiB of slots
constexpr uint64_t kMaxRecords = 1ull << 21;

[[noreturn]] void die(const std::string& what) {
  fflush(stdout);
  fprintf(stderr, "tablecheck: %s\n", what.c_str());
  fflush(stderr);
  _exit(1);  // no destructors: nothing more touches the device
}

#define CHK(call)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      die(std::string("HIP error ") + hipGetErrorString(e_) + " at line " + std::to_string(__LINE__) + " (" #call ")"); \
  } while (0)

// Blocks per group of the slab kernels: BfsEngine::slab_gy.
int slab_gy(int groups, uint64_t per) {
  constexpr int total = 2048;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>((per + kBlock - 1) / kBlock,
                                                       (uint64_t)std::max(1, total / std::max(1, groups))));
}

struct Reader {
  std::vector<uint64_t> w;
  size_t at = 0;
  bool more() const { return at < w.size(); }
  uint64_t next() {
    if (at >= w.size()) die("scenario ends inside an operation");
    return w[at++];
  }
  const uint64_t* take(uint64_t n) {
    if (n > w.size() - at) die("scenario ends inside an image");
    const uint64_t* p = w.data() + at;
    at += n;
    return p;
  }
};

void put_hex_bytes(const char* name, const uint8_t* p, size_t n) {
  static const char* hx = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (size_t i = 0; i < n; i++) {
    s[2 * i] = hx[p[i] >> 4];
    s[2 * i + 1] = hx[p[i] & 15];
  }
  printf("\"%s\":\"%s\"", name, s.c_str());
}
// 16 hex digits per word, most significant first
void put_hex_words(const char* name, const uint64_t* p, size_t n) {
  static const char* hx = "0123456789abcdef";
  std::string s(16 * n, '0');
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 16; k++) s[16 * i + k] = hx[(p[i] >> (60 - 4 * k)) & 15];
  printf("\"%s\":\"%s\"", name, s.c_str());
}

struct Dev {
  hipStream_t stream = nullptr;
  LevelCounters* ctr = nullptr;
  Table tbl{nullptr, 0, 0, 0};
  int b = -1;
  // the routed regions of one shard (slab_load)
  int W = 0, me = 0;
  uint64_t cs = 0, cap_fp = 0, cap_pk = 0;
  Fp *out_key = nullptr, *in_key = nullptr;
  uint32_t *out_pk = nullptr, *in_pk = nullptr;
  uint8_t *rep_out = nullptr, *rep_in = nullptr;
  RouteCounters* rc = nullptr;
  unsigned long long* nl_ctr = nullptr;

  void init() {
    if (stream) return;
    CHK(hipSetDevice(0));
    CHK(hipStreamCreate(&stream));
    CHK(hipMalloc(&ctr, sizeof(LevelCounters)));
    CHK(hipMalloc(&rc, sizeof(RouteCounters)));
    CHK(hipMalloc(&nl_ctr, 8));
  }
  void sync() { CHK(hipStreamSynchronize(stream)); }
  void need_table() {
    if (!tbl.slots) die("no table yet");
  }
  void zero_ctr() { CHK(hipMemsetAsync(ctr, 0, sizeof(LevelCounters), stream)); }
  void put_ctr() {
    LevelCounters c;
    CHK(hipMemcpy(&c, ctr, sizeof(c), hipMemcpyDeviceToHost));
    printf(",\"new_states\":%llu,\"err_table\":%llu", c.new_states, c.err_table);
  }
  void set_rc(const uint64_t* cnt, int nW) {
    static RouteCounters h;
    std::memset(&h, 0, sizeof(h));
    for (int d = 0; d < nW; d++)
      for (int q = 0; q < kRouteSegs; q++) h.out[rc_idx(d, q)] = cnt[d * kRouteSegs + q];
    CHK(hipMemcpyAsync(rc, &h, sizeof(h), hipMemcpyHostToDevice, stream));
    sync();  // h is reused
  }
};

void op_table(Dev& D, Reader& R) {
  const uint64_t b = R.next(), b0 = R.next(), lf = R.next();
  if (b > (uint64_t)kMaxLog2Buckets || b0 > b || lf > 1) die("table: bad arguments");
  D.init();
  if (D.tbl.slots) CHK(hipFree(D.tbl.slots));
  const uint64_t nb = 1ull << b;
  CHK(hipMalloc(&D.tbl.slots, nb * 64));
  CHK(hipMemsetAsync(D.tbl.slots, 0, nb * 64, D.stream));
  D.sync();
  D.tbl.bucket_mask = nb - 1;
  D.tbl.b0 = (int32_t)b0;
  D.tbl.load_first = (int32_t)lf;
  D.b = (int)b;
  printf("{\"op\":\"table\",\"b\":%d,\"b0\":%d,\"load_first\":%d}", D.b, D.tbl.b0, D.tbl.load_first);
}

void op_probe_remote(Dev& D, Reader& R) {
  const uint64_t n = R.next();
  if (n > kMaxRecords) die("probe_remote: too many records");
  const uint64_t* img = R.take(2 * n);
  D.need_table();
  std::vector<Fp> fps(n);
  for (uint64_t i = 0; i < n; i++) fps[i] = Fp{img[2 * i], img[2 * i + 1]};
  std::vector<uint8_t> rep(n);
  D.zero_ctr();
  if (n) {  // the engine launches nothing for a shard that received nothing
    Fp* d_in = nullptr;
    uint8_t* d_rep = nullptr;
    CHK(hipMalloc(&d_in, n * sizeof(Fp)));
    CHK(hipMalloc(&d_rep, n));
    CHK(hipMemcpyAsync(d_in, fps.data(), n * sizeof(Fp), hipMemcpyHostToDevice, D.stream));
    CHK(hipMemsetAsync(d_rep, 0xAA, n, D.stream));
    ProbeArgs pa;
    pa.in = d_in;
    pa.n = n;
    pa.table = D.tbl;
    pa.reply = d_rep;
    pa.ctr = D.ctr;
    const int blocks = (int)std::min<uint64_t>((n + kBlock - 1) / kBlock, 8192);
    hipLaunchKernelGGL(k_probe_remote, dim3(blocks), dim3(kBlock), 0, D.stream, pa);
    CHK(hipGetLastError());
    D.sync();
    CHK(hipMemcpy(rep.data(), d_rep, n, hipMemcpyDeviceToHost));
    CHK(hipFree(d_in));
    CHK(hipFree(d_rep));
  }
  D.sync();
  printf("{\"op\":\"probe_remote\",");
  put_hex_bytes("reply", rep.data(), n);
  D.put_ctr();
  printf("}");
}

template <class T>
void upload(Dev& D, T** dst, const uint64_t* img, uint64_t bytes) {
  if (*dst) CHK(hipFree(*dst));
  CHK(hipMalloc(dst, std::max<uint64_t>(bytes, 8)));
  CHK(hipMemcpyAsync(*dst, img, bytes, hipMemcpyHostToDevice, D.stream));
  D.sync();
}

void op_slab_load(Dev& D, Reader& R) {
  const uint64_t W = R.next(), me = R.next(), cs = R.next();
  if (W < 1 || W > (uint64_t)kMaxShards || me >= W || cs < 1 || cs > (1u << 16)) die("slab_load: bad arguments");
  D.init();
  D.W = (int)W;
  D.me = (int)me;
  D.cs = cs;
  D.cap_fp = kRouteHdr + (uint64_t)kRouteSegs * cs;
  D.cap_pk = pk_region_words(cs);
  const uint64_t key_words = 2 * W * D.cap_fp, pk_words = (W * D.cap_pk + 1) / 2;
  const uint64_t* ok = R.take(key_words);
  const uint64_t* ik = R.take(key_words);
  const uint64_t* op = R.take(pk_words);
  const uint64_t* ip = R.take(pk_words);
  upload(D, &D.out_key, ok, key_words * 8);
  upload(D, &D.in_key, ik, key_words * 8);
  upload(D, &D.out_pk, op, W * D.cap_pk * 4);
  upload(D, &D.in_pk, ip, W * D.cap_pk * 4);
  if (D.rep_out) CHK(hipFree(D.rep_out));
  if (D.rep_in) CHK(hipFree(D.rep_in));
  CHK(hipMalloc(&D.rep_out, W * D.cap_fp));
  CHK(hipMalloc(&D.rep_in, W * D.cap_fp));
  printf("{\"op\":\"slab_load\",\"cap_fp\":%llu,\"cap_pk\":%llu}", (unsigned long long)D.cap_fp,
         (unsigned long long)D.cap_pk);
}

void op_probe_slab(Dev& D, Reader& R) {
  const uint64_t packed = R.next(), with_reply = R.next();
  if (packed > 1 || with_reply > 1) die("probe_slab: bad arguments");
  D.need_table();
  if (!D.W) die("probe_slab: no regions yet");
  const uint64_t nrep = (uint64_t)D.W * D.cap_fp;
  D.zero_ctr();
  CHK(hipMemsetAsync(D.rep_out, 0xAA, nrep, D.stream));
  CHK(hipMemsetAsync(D.rep_in, 0xAA, nrep, D.stream));
  ProbeSlabArgs pa{};  // BfsEngine::sharded_fast
  pa.in = D.in_key;
  pa.in_pk = packed ? D.in_pk : nullptr;
  pa.self_pk = D.out_pk + (size_t)D.me * D.cap_pk;
  pa.cap_pk = D.cap_pk;
  pa.self = D.out_key + (size_t)D.me * D.cap_fp;
  pa.cap_fp = D.cap_fp;
  pa.cs = D.cs;
  pa.W = D.W;
  pa.me = D.me;
  pa.table = D.tbl;
  pa.reply = with_reply ? D.rep_out : nullptr;
  pa.self_reply = D.rep_in + (size_t)D.me * D.cap_fp;
  pa.ctr = D.ctr;
  const int groups = D.W * kRouteSegs;
  hipLaunchKernelGGL(k_probe_slab, dim3(groups, slab_gy(groups, D.cs)), dim3(kBlock), 0, D.stream, pa);
  CHK(hipGetLastError());
  D.sync();
  std::vector<uint8_t> ro(nrep), ri(nrep);
  CHK(hipMemcpy(ro.data(), D.rep_out, nrep, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(ri.data(), D.rep_in, nrep, hipMemcpyDeviceToHost));
  printf("{\"op\":\"probe_slab\",");
  put_hex_bytes("reply", ro.data(), nrep);
  printf(",");
  put_hex_bytes("self_reply", ri.data(), nrep);
  D.put_ctr();
  printf("}");
}

void op_rehash(Dev& D, Reader& R) {
  const uint64_t b2 = R.next();
  D.need_table();
  if (b2 > (uint64_t)kMaxLog2Buckets || b2 < (uint64_t)D.b) die("rehash: bad size");
  const uint64_t have = D.tbl.bucket_mask + 1, nb = 1ull << b2;
  unsigned long long* d_err = nullptr;
  CHK(hipMalloc(&d_err, 8));
  CHK(hipMemsetAsync(d_err, 0, 8, D.stream));
  Table to = D.tbl;  // BfsEngine::ensure_table
  to.bucket_mask = nb - 1;
  CHK(hipMalloc(&to.slots, nb * 64));
  CHK(hipMemsetAsync(to.slots, 0, nb * 64, D.stream));
  const int grid = (int)std::min<uint64_t>(8192, std::max<uint64_t>(1, have * 8 / kBlock));
  hipLaunchKernelGGL(k_rehash, dim3(grid), dim3(kBlock), 0, D.stream, D.tbl, to, d_err);
  CHK(hipGetLastError());
  D.sync();
  unsigned long long bad = 0;
  CHK(hipMemcpy(&bad, d_err, 8, hipMemcpyDeviceToHost));
  CHK(hipFree(d_err));
  CHK(hipFree(D.tbl.slots));
  D.tbl = to;
  D.b = (int)b2;
  printf("{\"op\":\"rehash\",\"b\":%d,\"err\":%llu}", D.b, bad);
}

void op_route_headers(Dev& D, Reader& R) {
  const uint64_t received = R.next(), with_pk = R.next(), with_zero = R.next();
  if (received > 1 || with_pk > 1 || with_zero > 1) die("route_headers: bad arguments");
  if (!D.W) die("route_headers: no regions yet");
  const int W = D.W;
  D.set_rc(R.take((uint64_t)W * kRouteSegs), W);
  const unsigned long long mark = 0xDEADBEEFCAFEF00Dull;
  CHK(hipMemcpyAsync(D.nl_ctr, &mark, 8, hipMemcpyHostToDevice, D.stream));
  D.sync();
  Fp* key = received ? D.in_key : D.out_key;
  uint32_t* pk = received ? D.in_pk : D.out_pk;
  hipLaunchKernelGGL(k_route_headers, dim3(1), dim3(kMaxShards * kRouteSegs), 0, D.stream,
                     (const RouteCounters*)D.rc, key, D.cap_fp, D.cs, W,
                     (unsigned long long*)(with_zero ? D.nl_ctr : nullptr), with_pk ? pk : (uint32_t*)nullptr, D.cap_pk);
  CHK(hipGetLastError());
  D.sync();
  unsigned long long z = 0;
  CHK(hipMemcpy(&z, D.nl_ctr, 8, hipMemcpyDeviceToHost));
  printf("{\"op\":\"route_headers\",\"zero_ctr\":%llu,\"key_hdr\":[", z);
  for (int d = 0; d < W; d++) {
    uint64_t h[kRouteSegs];
    CHK(hipMemcpy(h, key + (uint64_t)d * D.cap_fp, sizeof(h), hipMemcpyDeviceToHost));
    for (int q = 0; q < kRouteSegs; q++) printf("%s%llu", d + q ? "," : "", (unsigned long long)h[q]);
  }
  printf("],\"pk_hdr\":[");
  for (int d = 0; d < W; d++) {
    uint32_t h[2 * kRouteSegs];
    CHK(hipMemcpy(h, pk + (uint64_t)d * D.cap_pk, sizeof(h), hipMemcpyDeviceToHost));
    for (int q = 0; q < 2 * kRouteSegs; q++) printf("%s%u", d + q ? "," : "", h[q]);
  }
  printf("]}");
}

void op_new_list(Dev& D, Reader& R) {
  const uint64_t dev = R.next(), W = R.next(), cap = R.next(), cs = R.next();
  if (dev > 1 || W < 1 || W > (uint64_t)kMaxShards || cap < 1 || cap > kMaxRecords || W * cap > 4 * kMaxRecords)
    die("new_list: bad arguments");
  if (dev && (cs < 1 || kRouteHdr + (uint64_t)kRouteSegs * cs > cap)) die("new_list: regions larger than cap");
  D.init();
  NewListArgs na{};  // BfsEngine::launch_materialize
  if (dev) {
    D.set_rc(R.take(W * kRouteSegs), (int)W);
  } else {
    const uint64_t* cnt = R.take(kMaxShards);
    for (int d = 0; d < kMaxShards; d++) {
      if ((uint64_t)d < W && cnt[d] > cap) die("new_list: a count past cap");
      na.cnt[d] = cnt[d];
    }
  }
  const uint64_t nrep = W * cap;
  const uint64_t* img = R.take((nrep + 7) / 8);
  uint8_t* d_rep = nullptr;
  uint64_t* d_list = nullptr;
  CHK(hipMalloc(&d_rep, nrep));
  CHK(hipMalloc(&d_list, nrep * 8));
  CHK(hipMemcpyAsync(d_rep, img, nrep, hipMemcpyHostToDevice, D.stream));
  CHK(hipMemsetAsync(d_list, 0xFF, nrep * 8, D.stream));
  CHK(hipMemsetAsync(D.nl_ctr, 0, 8, D.stream));
  na.reply = d_rep;
  na.cap = cap;
  na.W = (int32_t)W;
  na.dev_cnt = dev ? D.rc : nullptr;
  na.cs = cs;
  na.list = d_list;
  na.n_list = D.nl_ctr;
  const uint64_t per = dev ? cs : cap;
  const int groups = dev ? (int)W * kRouteSegs : (int)W;
  const int gy = slab_gy(groups, per);
  hipLaunchKernelGGL(k_new_list, dim3(groups, gy), dim3(kBlock), 0, D.stream, na);
  CHK(hipGetLastError());
  D.sync();
  unsigned long long n_list = 0;
  CHK(hipMemcpy(&n_list, D.nl_ctr, 8, hipMemcpyDeviceToHost));
  std::vector<uint64_t> list(nrep);
  CHK(hipMemcpy(list.data(), d_list, nrep * 8, hipMemcpyDeviceToHost));
  CHK(hipFree(d_rep));
  CHK(hipFree(d_list));
  const uint64_t shown = std::min<uint64_t>(n_list, nrep);
  uint64_t stray = 0;  // list words written past n_list
  for (uint64_t i = shown; i < nrep; i++) stray += list[i] != ~0ull;
  printf("{\"op\":\"new_list\",\"grid_y\":%d,\"n_list\":%llu,\"stray\":%llu,\"list\":[", gy, n_list,
         (unsigned long long)stray);
  for (uint64_t i = 0; i < shown; i++) printf("%s%llu", i ? "," : "", (unsigned long long)list[i]);
  printf("]}");
}

void op_dump(Dev& D) {
  D.need_table();
  const uint64_t n = (D.tbl.bucket_mask + 1) * 8;
  std::vector<uint64_t> s(n);
  D.sync();
  CHK(hipMemcpy(s.data(), D.tbl.slots, n * 8, hipMemcpyDeviceToHost));
  printf("{\"op\":\"dump\",\"b\":%d,", D.b);
  put_hex_words("slots", s.data(), n);
  printf("}");
}

void op_layout(Reader& R) {
  const uint64_t n = R.next();
  if (n > kMaxRecords) die("layout: too many entries");
  const uint64_t* e = R.take(7 * n);
  std::vector<uint64_t> key0(n), home(n), rehome(n);
  for (uint64_t k = 0; k < n; k++, e += 7) {
    if (e[0] > (uint64_t)kKeyBits || e[1] > (uint64_t)kKeyBits || e[2] > (uint64_t)kKeyBits) die("layout: bad sizes");
    const Table from{nullptr, (1ull << e[1]) - 1, (int32_t)e[0], 0}, to{nullptr, (1ull << e[2]) - 1, (int32_t)e[0], 0};
    const Fp f{e[3], e[4]};
    key0[k] = table_key0(from, f);
    home[k] = table_home(from, f);
    rehome[k] = table_rehome(from, to, e[5], e[6]);
  }
  printf("{\"op\":\"layout\",");
  put_hex_words("key0", key0.data(), n);
  printf(",");
  put_hex_words("home", home.data(), n);
  printf(",");
  put_hex_words("rehome", rehome.data(), n);
  printf("}");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: tablecheck <scenario file>\n"), 2;
  Reader R;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "tablecheck: cannot open %s\n", argv[1]), 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 8 || bytes % 8) return fprintf(stderr, "tablecheck: not a scenario\n"), 2;
    R.w.resize((size_t)bytes / 8);
    if (fread(R.w.data(), 8, R.w.size(), f) != R.w.size()) return fprintf(stderr, "tablecheck: short read\n"), 2;
    fclose(f);
  }
  if (R.next() != kMagic) return fprintf(stderr, "tablecheck: not a scenario\n"), 2;
  Dev D;
  printf("{\"results\":[");
  bool first = true;
  while (R.more()) {
    const uint64_t op = R.next();
    if (!first) printf(",");
    first = false;
    switch (op) {
      case 1: op_table(D, R); break;
      case 2: op_probe_remote(D, R); break;
      case 3: op_slab_load(D, R); break;
      case 4: op_probe_slab(D, R); break;
      case 5: op_rehash(D, R); break;
      case 6: op_route_headers(D, R); break;
      case 7: op_new_list(D, R); break;
      case 8: op_dump(D); break;
      case 9: op_layout(R); break;
      default: die("unknown operation " + std::to_string(op));
    }
  }
  printf("]}\n");
  fflush(stdout);
  if (D.stream) CHK(hipStreamSynchronize(D.stream));
  _exit(0);  // the process ends here: device memory goes with it
}
