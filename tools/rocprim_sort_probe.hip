// Yardstick for the segmented radix sort of efa_pmmean.hip: rocprim::radix_sort_keys on the same number of 64-bit and
// 32-bit keys, full-range random bits, one array (rocPRIM's device-wide sort is not segmented; its segmented sort is a different
// algorithm, one workgroup per segment).  Stand-alone, not linked into the library:
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/rocprim_sort_probe.hip -o tools/rocprim_sort_probe
//     tools/rocprim_sort_probe <keys> [rounds]
// Prints one JSON line: the median device time (HIP events) of `rounds` sorts after one warm-up, per key width.
#include <cstring>  // (rocPRIM's texture iterator calls memset without it)

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(expr)                                                                       \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      std::fprintf(stderr, "%s failed: %s\n", #expr, hipGetErrorString(e_));              \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

template <typename K>
__global__ void k_fill(K* out, size_t n, unsigned long long seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned long long z = (i + seed) * 0x9E3779B97F4A7C15ull;  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    out[i] = (K)(z ^ (z >> 31));
  }
}

template <typename K>
int run(size_t n, int rounds, double* median_ms, int* sorted_ok) {
  K *in = nullptr, *out = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  CHECK(hipMalloc(&in, n * sizeof(K)));
  CHECK(hipMalloc(&out, n * sizeof(K)));
  CHECK(rocprim::radix_sort_keys(nullptr, tmp_bytes, in, out, n));
  CHECK(hipMalloc(&tmp, tmp_bytes));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  std::vector<float> ms;
  for (int r = 0; r <= rounds; ++r) {
    hipLaunchKernelGGL(k_fill<K>, dim3(2048), dim3(256), 0, 0, in, n, 1234ull + r);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(a, 0));
    CHECK(rocprim::radix_sort_keys(tmp, tmp_bytes, in, out, n));
    CHECK(hipEventRecord(b, 0));
    CHECK(hipEventSynchronize(b));
    float t = 0.f;
    CHECK(hipEventElapsedTime(&t, a, b));
    if (r > 0) ms.push_back(t);
  }
  std::sort(ms.begin(), ms.end());
  *median_ms = ms[ms.size() / 2];
  const size_t m = std::min<size_t>(n, 1 << 20);
  std::vector<K> h(m);
  CHECK(hipMemcpy(h.data(), out, m * sizeof(K), hipMemcpyDeviceToHost));
  *sorted_ok = std::is_sorted(h.begin(), h.end()) ? 1 : 0;
  CHECK(hipFree(tmp));
  CHECK(hipFree(in));
  CHECK(hipFree(out));
  CHECK(hipEventDestroy(a));
  CHECK(hipEventDestroy(b));
  return 0;
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : (size_t)1 << 24;
  const int rounds = argc > 2 ? std::atoi(argv[2]) : 5;
  if (n < 1 || rounds < 1) return 2;
  double ms64 = 0.0, ms32 = 0.0;
  int ok64 = 0, ok32 = 0;
  if (run<unsigned long long>(n, rounds, &ms64, &ok64)) return 1;
  if (run<unsigned int>(n, rounds, &ms32, &ok32)) return 1;
  std::printf("{\"keys\": %zu, \"rounds\": %d, \"u64_ms\": %.4f, \"u32_ms\": %.4f, \"u64_keys_per_s\": %.4g, \"u32_keys_per_s\": %.4g, "
              "\"sorted\": %d}\n",
              n, rounds, ms64, ms32, n / (ms64 * 1e-3), n / (ms32 * 1e-3), ok64 && ok32);
  return ok64 && ok32 ? 0 : 3;
}
