// Experiment (not part of the library): the face pick of nsdp_amd/csrc/mesh_sample.hip -- a binary search over F thresholds per
// row -- ALONE, with and without a coarse level of the thresholds staged in LDS.  One lane per row, 256-lane workgroups, B samples
// over four threshold rows of F = 40 000 sorted random values; a row draws r from a hash.  "plain" is the kernel's search; the
// staged forms fill a coarse level of 64 / 256 / 1024 entries per workgroup from global memory, search it in LDS and then search
// the segment it names.  The four forms alternate inside one loop of 20 timed rounds (three warm-up rounds before), median and
// range per form; the staged results are compared with the plain ones row by row.  profiles/mesh_store.txt holds a run; DESIGN.md
// section 4m and docs/EXPERIMENTS.md say what was decided from it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/search_lds_experiment.hip -o search_lds_experiment && ./search_lds_experiment
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e = (x);                                                           \
    if (e != hipSuccess) {                                                        \
      std::printf("%s: %s\n", #x, hipGetErrorString(e));                          \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

__host__ __device__ inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void plain(const uint32_t *__restrict__ T, int F, int rows, uint32_t key, int *__restrict__ out) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= rows) return;
  const uint32_t *t = T + static_cast<size_t>(blockIdx.y % 4) * F;
  const uint32_t r = mix32(mix32(j ^ key) + blockIdx.y) >> 1;
  int lo = 0, hi = F;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] > r) hi = mid; else lo = mid + 1;
  }
  out[static_cast<size_t>(blockIdx.y) * rows + j] = min(lo, F - 1);
}

// coarse level: kCoarse entries c[k] = T[seg_end(k) - 1], seg_end(k) = (k + 1) * F / kCoarse; search c in LDS, then the segment
template <int kCoarse>
__global__ __launch_bounds__(kThreads) void staged(const uint32_t *__restrict__ T, int F, int rows, uint32_t key, int *__restrict__ out) {
  __shared__ uint32_t c[kCoarse];
  const uint32_t *t = T + static_cast<size_t>(blockIdx.y % 4) * F;
  for (int k = threadIdx.x; k < kCoarse; k += kThreads) {
    const int end = static_cast<int>((static_cast<long long>(k + 1) * F) / kCoarse);
    c[k] = t[max(end - 1, 0)];
  }
  __syncthreads();
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= rows) return;
  const uint32_t r = mix32(mix32(j ^ key) + blockIdx.y) >> 1;
  int a = 0, b = kCoarse;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (c[mid] > r) b = mid; else a = mid + 1;
  }
  const int seg = min(a, kCoarse - 1);
  int lo = static_cast<int>((static_cast<long long>(seg) * F) / kCoarse), hi = static_cast<int>((static_cast<long long>(seg + 1) * F) / kCoarse);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] > r) hi = mid; else lo = mid + 1;
  }
  out[static_cast<size_t>(blockIdx.y) * rows + j] = min(lo, F - 1);
}

int main() {
  const int F = 40000, B = 32, rounds = 20;
  std::vector<uint32_t> T(4 * static_cast<size_t>(F));
  uint32_t s = 12345;
  for (int f4 = 0; f4 < 4; ++f4) {
    uint32_t *t = T.data() + static_cast<size_t>(f4) * F;
    for (int f = 0; f < F; ++f) t[f] = (s = mix32(s + f)) >> 1;
    std::sort(t, t + F);
    t[F - 1] = 1u << 31;
  }
  uint32_t *dT;
  int *o1, *o2;
  const int max_rows = 40960;
  CHECK(hipMalloc(&dT, T.size() * 4));
  CHECK(hipMalloc(&o1, static_cast<size_t>(B) * max_rows * 4));
  CHECK(hipMalloc(&o2, static_cast<size_t>(B) * max_rows * 4));
  CHECK(hipMemcpy(dT, T.data(), T.size() * 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (int rows : {1280, 10240, 40960}) {
    const dim3 grid((rows + kThreads - 1) / kThreads, B);
    std::vector<float> tp, t64, t256, t1024;
    for (int r = 0; r < rounds + 3; ++r) {
      float ms;
      const uint32_t key = 77 + r;
      auto time = [&](auto launch, std::vector<float> &into) {
        CHECK(hipEventRecord(e0));
        launch();
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 3) into.push_back(ms);
      };
      time([&] { hipLaunchKernelGGL(plain, grid, dim3(kThreads), 0, 0, dT, F, rows, key, o1); }, tp);
      time([&] { hipLaunchKernelGGL(staged<64>, grid, dim3(kThreads), 0, 0, dT, F, rows, key, o2); }, t64);
      time([&] { hipLaunchKernelGGL(staged<256>, grid, dim3(kThreads), 0, 0, dT, F, rows, key, o2); }, t256);
      time([&] { hipLaunchKernelGGL(staged<1024>, grid, dim3(kThreads), 0, 0, dT, F, rows, key, o2); }, t1024);
      CHECK(hipGetLastError());
    }
    std::vector<int> h1(static_cast<size_t>(B) * rows), h2(h1.size());
    CHECK(hipMemcpy(h1.data(), o1, h1.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h2.data(), o2, h2.size() * 4, hipMemcpyDeviceToHost));
    size_t differ = 0;
    for (size_t i = 0; i < h1.size(); ++i) differ += h1[i] != h2[i];
    auto stats = [](std::vector<float> v, const char *name) {
      std::sort(v.begin(), v.end());
      std::printf("  %-22s median %7.4f ms   range %7.4f .. %7.4f\n", name, v[v.size() / 2], v.front(), v.back());
    };
    std::printf("search alone, F = %d, B = %d x %d rows (results differ at %zu rows):\n", F, B, rows, differ);
    stats(tp, "plain (global only)");
    stats(t64, "LDS coarse level 64");
    stats(t256, "LDS coarse level 256");
    stats(t1024, "LDS coarse level 1024");
  }
  return 0;
}
