// tests/devcheck/containscheck.hip -- TEST TOOL, not part of the product.
//
// table_contains (fingerprint.hpp) in isolation, beside the product's own table_insert: a zeroed
// table is filled with one table_insert per record, dumped, asked with one table_contains per
// query, and dumped again. It judges nothing: tests/test_gpu_table_contains.py makes the records
// and compares the answers with tests/table_model.py.
//
// usage: containscheck <scenario file>
//
// The scenario is little-endian 64-bit words: kMagic, b (a table of 2^b buckets), b0, load_first,
// n_fill, n_query, then n_fill records (hi, lo) and n_query records (hi, lo). One JSON object:
// "insert" (one InsertRc byte per filled record), "contains" (one byte per query, pre-filled with
// 0xAA), "before" / "after" (every slot word around the lookups, 16 hex digits each).
// Every HIP call is checked: the first error is printed and ends the program, non-zero, with
// nothing started after it.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../dslabs_amd/csrc/fingerprint.hpp"

using namespace dsl;

namespace {

constexpr uint64_t kMagic = 0x3130534e49544e43ull;  // "CNTINS01"
constexpr int kMaxLog2Buckets = 16;
constexpr uint64_t kMaxRecords = 1ull << 20;
constexpr int kThreads = 256;

[[noreturn]] void die(const std::string& what) {
  fflush(stdout);
  fprintf(stderr, "containscheck: %s\n", what.c_str());
  fflush(stderr);
  _exit(1);  // no destructors: nothing more touches the device
}

#define CHK(call)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      die(std::string("HIP error ") + hipGetErrorString(e_) + " at line " + std::to_string(__LINE__) + " (" #call ")"); \
  } while (0)

__global__ void __launch_bounds__(kThreads) k_fill(Table t, const Fp* in, uint64_t n, uint8_t* rc) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) rc[i] = (uint8_t)table_insert(t, in[i]);
}

__global__ void __launch_bounds__(kThreads) k_contains(Table t, const Fp* in, uint64_t n, uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = table_contains(t, in[i]) ? 1 : 0;
}

void put_hex_bytes(const char* name, const uint8_t* p, size_t n) {
  static const char* hx = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (size_t i = 0; i < n; i++) {
    s[2 * i] = hx[p[i] >> 4];
    s[2 * i + 1] = hx[p[i] & 15];
  }
  printf("\"%s\":\"%s\"", name, s.c_str());
}
void put_hex_words(const char* name, const uint64_t* p, size_t n) {
  static const char* hx = "0123456789abcdef";
  std::string s(16 * n, '0');
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 16; k++) s[16 * i + k] = hx[(p[i] >> (60 - 4 * k)) & 15];
  printf("\"%s\":\"%s\"", name, s.c_str());
}

// n records on the device, from 2 n words; nullptr for none
Fp* upload(const uint64_t* img, uint64_t n, hipStream_t st) {
  if (!n) return nullptr;
  std::vector<Fp> fps(n);
  for (uint64_t i = 0; i < n; i++) fps[i] = Fp{img[2 * i], img[2 * i + 1]};
  Fp* d = nullptr;
  CHK(hipMalloc(&d, n * sizeof(Fp)));
  CHK(hipMemcpyAsync(d, fps.data(), n * sizeof(Fp), hipMemcpyHostToDevice, st));
  CHK(hipStreamSynchronize(st));  // fps leaves scope
  return d;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: containscheck <scenario file>");
  FILE* f = fopen(argv[1], "rb");
  if (!f) die("cannot open the scenario");
  std::vector<uint64_t> w;
  uint64_t x;
  while (fread(&x, 8, 1, f) == 1) w.push_back(x);
  fclose(f);
  if (w.size() < 6 || w[0] != kMagic) die("not a scenario");
  const uint64_t b = w[1], b0 = w[2], lf = w[3], nf = w[4], nq = w[5];
  if (b > (uint64_t)kMaxLog2Buckets || b0 > b || lf > 1 || nf > kMaxRecords || nq > kMaxRecords ||
      w.size() != 6 + 2 * nf + 2 * nq)
    die("bad scenario");
  hipStream_t st;
  CHK(hipSetDevice(0));
  CHK(hipStreamCreate(&st));
  const uint64_t nslots = 8ull << b;
  Table t{nullptr, (1ull << b) - 1, (int32_t)b0, (int32_t)lf};
  CHK(hipMalloc(&t.slots, nslots * 8));
  CHK(hipMemsetAsync(t.slots, 0, nslots * 8, st));
  Fp* d_fill = upload(w.data() + 6, nf, st);
  Fp* d_query = upload(w.data() + 6 + 2 * nf, nq, st);
  uint8_t *d_rc = nullptr, *d_out = nullptr;
  CHK(hipMalloc(&d_rc, nf + 1));
  CHK(hipMalloc(&d_out, nq + 1));
  CHK(hipMemsetAsync(d_rc, 0xAA, nf + 1, st));
  CHK(hipMemsetAsync(d_out, 0xAA, nq + 1, st));
  std::vector<uint8_t> rc(nf), out(nq);
  std::vector<uint64_t> before(nslots), after(nslots);
  if (nf) {
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((nf + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, t, d_fill, nf, d_rc);
    CHK(hipGetLastError());
  }
  CHK(hipStreamSynchronize(st));
  CHK(hipMemcpy(before.data(), t.slots, nslots * 8, hipMemcpyDeviceToHost));
  if (nq) {
    hipLaunchKernelGGL(k_contains, dim3((unsigned)((nq + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, t, d_query, nq,
                       d_out);
    CHK(hipGetLastError());
  }
  CHK(hipStreamSynchronize(st));
  CHK(hipMemcpy(after.data(), t.slots, nslots * 8, hipMemcpyDeviceToHost));
  if (nf) CHK(hipMemcpy(rc.data(), d_rc, nf, hipMemcpyDeviceToHost));
  if (nq) CHK(hipMemcpy(out.data(), d_out, nq, hipMemcpyDeviceToHost));
  printf("{");
  put_hex_bytes("insert", rc.data(), nf);
  printf(",");
  put_hex_bytes("contains", out.data(), nq);
  printf(",");
  put_hex_words("before", before.data(), nslots);
  printf(",");
  put_hex_words("after", after.data(), nslots);
  printf("}\n");
  fflush(stdout);
  _exit(0);
}
